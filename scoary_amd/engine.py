"""Device-side association engine: thin Python over the C-ABI.

PyTorch-ROCm is used for device memory and streams only; every computation of
the hot path happens in libscoary_hip.so (scoary_amd/csrc/scoary_*.hip).
"""
import ctypes

import numpy as np

from . import _abi


def _torch():
    import torch
    return torch


def pack_bits_rows(dense01):
    """Host helper (spec S1): (R, N) 0/1 array -> (R, W64) uint64 rows, bit i
    of word w = column 64*w+i.  Pure numpy; this is input preparation, the
    same bit-packing the CSV reader produces."""
    dense01 = np.ascontiguousarray(dense01, dtype=np.uint8)
    R, N = dense01.shape
    W = (N + 63) // 64
    by = np.packbits(dense01, axis=1, bitorder="little")
    out = np.zeros((R, W * 8), dtype=np.uint8)
    out[:, :by.shape[1]] = by
    return out.view("<u8")


class GeneMatrix:
    """The bit-packed gene presence/absence matrix resident in HBM (tiled)."""

    def __init__(self, tiled, G, N):
        self.tiled = tiled      # torch.int32 [Qp, Gp, 4]
        self.G = int(G)
        self.N = int(N)
        self.lists = None       # GeneLists, for the list-driven permutation kernel
        # the tables of the last minp(..., plan=...) on this matrix, one slot per kind of table (engine._minp_batches):
        # "fisher" = the p tables, "cmh" = the CMH tables of a strata plan.  A step with both keeps both.
        self.minp_caches = {}

    @property
    def minp_cache(self):
        """The slot of Fisher's p tables (None: nothing kept)."""
        return self.minp_caches.get("fisher")

    @minp_cache.setter
    def minp_cache(self, slot):
        if slot is None:
            self.minp_caches.pop("fisher", None)
        else:
            self.minp_caches["fisher"] = slot


class ListMemoryError(_abi.ScoaryHipError):
    """The index lists of a gene matrix would not fit the memory budget (build_lists): the
    caller falls back to the dense permutation kernels, which need no lists."""


class GeneLists:
    """Minority index lists of a gene matrix on the device (scoary_lists_plan / _fill).
    start / ngroups: int32 [G] per list slot, or [segments, G] for N > 20479.
    panels: the slots' minority rows as matrix-core operands (scoary_mfma_panels_build; N <= 2048), or
    None; block_start: host int64 array, index entries in front of every 256-slot block (and the
    total last); routes: k_split per (routing mode, T, P), a host-side cache; N: the isolates of the matrix."""

    def __init__(self, idx, start, ngroups, order, flipped, entries, N):
        self.idx, self.start, self.ngroups = idx, start, ngroups
        self.order, self.flipped, self.entries, self.N = order, flipped, entries, int(N)
        self.panels, self.block_start, self.routes = None, None, {}


class MinpTables:
    """The p tables of a group of traits (scoary_minp_plan / _fill, spec S7): tab float64 [entries] holds
    p_tg(a) for every overlap count a of the support of (trait, gene), CSR-style: off int64 [T * G + 1], lo
    int32 [T, G] = the smallest a of the support; tab[off[t G + g] + a - lo[t, g]] = p_tg(a)."""

    def __init__(self, off, lo, tab, entries):
        self.off, self.lo, self.tab, self.entries = off, lo, tab, int(entries)


class TableSource:
    """Where a Westfall-Young pass (minp / minp_stepdown) takes its tables and observed values from: ``kind`` and
    ``key`` name the tables in genes.minp_caches (Fisher's p tables depend on the traits alone, key None; the CMH
    tables on the strata plan as well), ``build(t0, t1)`` -> the MinpTables of the traits [t0, t1), ``observed(t0,
    t1, tables)`` -> float64 [t1 - t0, G], the value every gene of those traits is ranked and counted by."""

    def __init__(self, kind, key, build, observed):
        self.kind, self.key, self.build, self.observed = kind, key, build, observed


class TraitPlan:
    """What the counts need that depends on the traits alone (scoary_trait_plan): margins
    int32 [T, 2] = (positives, valid isolates), mask_class int32 [T] = first trait OF THE SAME PASS with the same
    validity row, buf = the opaque plan buffer (class slots per pass + the label / validity
    rows gathered quad-major).  Built once per trait set; valid for exactly the traits / masks
    tensors it was built from (a snapshot: later in-place changes of them are not seen)."""

    def __init__(self, margins, mask_class, buf, traits, masks, N):
        self.margins, self.mask_class, self.buf, self.N = margins, mask_class, buf, int(N)
        # strong references: the memory the plan describes cannot be recycled for other data
        # while the plan lives, and `is` identifies the tensors (an address can be reused);
        # _version sees in-place edits made through torch after the snapshot
        self.traits, self.masks = traits, masks
        self.versions = (traits._version, masks._version)

    def fits(self, traits, masks):
        return (traits is self.traits and masks is self.masks
                and self.versions == (traits._version, masks._version))


class StrataPlan:
    """Strata for within-stratum label shuffles (spec S9; engine.strata_plan): strata int16 [N] (uint16 bit
    pattern) = the stratum of every isolate, members int32 [N] = the isolates by (stratum, index), offsets int32
    [S + 1] = the first member of every stratum, smargins int32 [T, S, 2] = (positives, valid isolates) of every
    (trait, stratum) -- device tensors -- and S, N, T; sizes = the host array of the S stratum sizes.  Valid for
    exactly the trait / mask rows it was built from."""

    def __init__(self, strata, members, offsets, smargins, S, N, sizes, checked=False):
        self.strata, self.members, self.offsets, self.smargins = strata, members, offsets, smargins
        self.S, self.N, self.T, self.sizes = int(S), int(N), int(smargins.shape[0]), sizes
        if not checked:
            # the library takes members and offsets as device arrays and cannot look at them: one host copy, here,
            # whoever built the plan -- the offsets run from 0 to N and the members are the isolates, each once
            off = offsets.cpu().numpy().astype(np.int64)
            mem = members.cpu().numpy().astype(np.int64)
            if off.shape != (self.S + 1,) or off[0] != 0 or off[-1] != self.N or (np.diff(off) < 0).any():
                raise ValueError("StrataPlan: the stratum offsets must rise from 0 to N = %d in S + 1 = %d entries"
                                 % (self.N, self.S + 1))
            if mem.shape != (self.N,) or not np.array_equal(np.sort(mem), np.arange(self.N)):
                raise ValueError("StrataPlan: members must hold every isolate 0 .. N - 1 exactly once")

    def rows(self, t0, t1):
        """The plan of the traits [t0, t1) alone (a view: the trait groups of minp())."""
        if t0 == 0 and t1 == self.T:
            return self
        return StrataPlan(self.strata, self.members, self.offsets, self.smargins[t0:t1], self.S, self.N, self.sizes,
                          checked=True)


class RankPlan:
    """The quantitative traits of a rank-sum step (spec S15; AssociationEngine.ranksum_plan): ``rc`` int16 [T, N]
    = the centred doubled midranks (0 where the value is missing), ``valid`` the validity rows (vecrows, int32
    [T, Wp]) and ``tiesum`` int64 [T] on the device; ``n``, ``tiesum_host`` and ``tie_groups`` (groups of two or
    more equal values) per trait and ``rc_host`` / ``valid_host`` (bool [T, N]) on the host."""

    def __init__(self, rc, valid, tiesum, rc_host, valid_host, n, tiesum_host, tie_groups, values_host=None):
        self.rc, self.valid, self.tiesum = rc, valid, tiesum
        self.rc_host, self.valid_host = rc_host, valid_host
        self.n, self.tiesum_host, self.tie_groups = n, tiesum_host, tie_groups
        self.T, self.N = (int(x) for x in rc_host.shape)
        self.values_host = values_host      # the values themselves, for the sorted rows of spec S19
        self.shift_plan = None              # ranksum_shift's RankShiftPlan, made when it is first asked for


class CategoricalPlan:
    """The categorical traits of a chi-square step (spec S20; AssociationEngine.categorical_plan): ``codes`` int16
    [T, N] (class 1 .. K, 0 = missing), ``valid`` the validity rows (vecrows), ``nk`` int32 [T, 8] and ``w`` (the
    limbs (low, high) of lcm{n_k > 0} / n_k, uint64 [T, 8, 2] held as int64) on the device; ``codes_host``,
    ``valid_host`` (bool [T, N]), ``n`` int64 [T], ``nk_host`` int64 [T, 8], ``classes`` (K' per trait, int64 [T]),
    ``weights`` (Python ints, [T][8]) and ``K`` (the largest code) on the host."""

    def __init__(self, codes, valid, nk, w, codes_host, valid_host, n, nk_host, classes, weights, K):
        self.codes, self.valid, self.nk, self.w = codes, valid, nk, w
        self.codes_host, self.valid_host = codes_host, valid_host
        self.n, self.nk_host, self.classes, self.weights, self.K = n, nk_host, classes, weights, K
        self.T, self.N = (int(x) for x in codes_host.shape)


CATEGORICAL_MAX_CLASSES = _abi.CATEGORICAL_MAX_CLASSES


def categorical_host(codes):
    """Host side of spec S20: integer codes [T, N] (0 = missing, classes from 1) -> (codes int16 [T, N], valid bool
    [T, N], n int64 [T], nk int64 [T, 8], K' int64 [T], weights [T][8] of Python ints = lcm{n_k > 0} / n_k, 0 for an
    empty class, and the same as limbs uint64 [T, 8, 2] (low, high))."""
    import math
    codes = np.ascontiguousarray(codes)
    if codes.ndim != 2 or codes.dtype.kind not in "iu":
        raise ValueError("categorical_plan: codes must be a [T, N] array of integers")
    if codes.size and (codes.min() < 0 or codes.max() > CATEGORICAL_MAX_CLASSES):
        raise ValueError("categorical_plan: a code is 0 (missing) or a class 1 .. %d" % CATEGORICAL_MAX_CLASSES)
    codes = codes.astype(np.int16)
    T = codes.shape[0]
    nk = np.stack([np.bincount(row, minlength=CATEGORICAL_MAX_CLASSES + 1)[1:] for row in codes]).astype(np.int64) \
        if T else np.zeros((0, CATEGORICAL_MAX_CLASSES), dtype=np.int64)
    weights, limbs = [], np.zeros((T, CATEGORICAL_MAX_CLASSES, 2), dtype=np.uint64)
    for t in range(T):
        lcm = 1
        for x in nk[t]:
            if x:
                lcm = lcm * int(x) // math.gcd(lcm, int(x))
        weights.append([lcm // int(x) if x else 0 for x in nk[t]])
        for k, wk in enumerate(weights[t]):
            limbs[t, k] = (wk & 0xFFFFFFFFFFFFFFFF, wk >> 64)
    return codes, codes != 0, nk.sum(axis=1), nk, (nk > 0).sum(axis=1), weights, limbs


class GcmhPlan:
    """The categorical traits of a generalized CMH step over strata (spec S21; AssociationEngine.gcmh_plan).  On the
    device: ``codes`` int16 [T, N] (class 1 .. K, 0 = missing), ``l`` int16 [T, N] = the codes of the labelled isolates
    by (stratum, isolate), ``valid`` the validity rows (vecrows), ``nk`` int32 [T, 8], ``nsk`` int32 [T, S, 8] (the
    class sizes inside every stratum), ``strata`` int16 [N] (uint16 bit pattern) and ``members`` int32 [N].  On the
    host: codes_host, strata_host int64 [N], n int64 [T], nk_host int64 [T, 8], nsk_host int64 [T, S, 8], ``classes``
    (K' per trait) and ``K`` (the largest code)."""

    def __init__(self, dev, codes_host, strata_host, S, n, nk_host, nsk_host, classes, K):
        self.codes, self.l, self.valid, self.nk, self.nsk, self.strata, self.members = dev
        self.codes_host, self.strata_host, self.S = codes_host, strata_host, int(S)
        self.n, self.nk_host, self.nsk_host, self.classes, self.K = n, nk_host, nsk_host, classes, K
        self.T, self.N = (int(x) for x in codes_host.shape)


GCMH_FORM = 35                                    # scoary_gcmh_form_doubles(): E[7], f[21], invp[7]


def gcmh_host(codes, strata, S):
    """Host side of spec S21 on top of categorical_host: (codes int16 [T, N], valid bool [T, N], n, nk, K' as there,
    nsk int64 [T, S, 8], l int16 [T, N] = the codes of the labelled isolates by (stratum, isolate), zeros behind)."""
    codes, valid, n, nk, classes, _weights, _limbs = categorical_host(codes)
    T, N = codes.shape
    nsk = np.zeros((T, S, CATEGORICAL_MAX_CLASSES), dtype=np.int64)
    l = np.zeros((T, N), dtype=np.int16)
    order = np.argsort(strata, kind="stable")
    for t in range(T):
        who = order[valid[t, order]]
        l[t, :who.size] = codes[t, who]
        np.add.at(nsk[t], (strata[who], codes[t, who].astype(np.int64) - 1), 1)
    return codes, valid, n, nk, classes, nsk, l


class ScorePlan:
    """The null models of a score-test step (spec S24; AssociationEngine.score_plan), ``kind`` "logistic" or "linear"
    with q = 1 + covariates design columns.  On the device: ``rows`` float64 [T, q + 1, N] (row 0 the residuals r_i,
    row 1 + j the weighted design column w_i x_ij; all zero at an isolate outside the trait's valid set), ``valid``
    the validity rows (vecrows), ``chol`` float64 [T, q (q + 1) / 2] (the lower Cholesky factor of A packed by rows)
    and ``rss`` float64 [T] (the null model's residual sum of squares, 0 for the logistic kind).  On the host: the
    same as rows_host, valid_host (bool [T, N]), chol_host, rss_host, ``n`` int64 [T], ``coef`` float64 [T, q] (the
    null model's coefficients on the scaled columns) and ``skipped`` (per trait None, or why S24 refuses its null
    model: a key of SCORE_SKIPS; such a trait has no valid isolate and every gene of it is untestable).  For spec S25:
    ``spa_rows_host`` float64 [T, q + 1, N] (row 0 the fitted mu_i, row 1 + j the design column x_ij) where the plan's
    maker gave mu and design, else None, and ``spa_rows``, the same on the device from the first
    AssociationEngine.score_spa on (None before: a run without it moves no byte of them)."""

    def __init__(self, dev, host, kind, q):
        self.rows, self.valid, self.chol, self.rss = dev
        self.rows_host, self.valid_host, self.chol_host, self.rss_host = (host[k] for k in ("rows", "valid", "chol",
                                                                                            "rss"))
        self.n, self.coef, self.skipped = host["n"], host["coef"], host["skipped"]
        self.kind, self.q = kind, int(q)
        self.T, self.N = (int(x) for x in self.valid_host.shape)
        self.spa_rows = self.spa_rows_host = None
        if host.get("mu") is not None and host.get("design") is not None:
            self.spa_rows_host = np.ascontiguousarray(
                np.concatenate([np.asarray(host["mu"], dtype=np.float64)[:, None, :],
                                np.asarray(host["design"], dtype=np.float64)], axis=1))


SCORE_MAX_COVARIATES = _abi.SCORE_MAX_COVARIATES
SCORE_KINDS = ("logistic", "linear")
# why S24 refuses the null model of a trait, in the order the rules are tried
SCORE_SKIPS = {
    "few": "it has %d isolates with a value and every covariate, the model of %d columns needs more than %d",
    "constant": "a covariate is constant over its %d isolates with a value and every covariate",
    "one_class": "all of its %d isolates with a value and every covariate are in one class",
    "collinear": "the covariates are collinear over its isolates with a value and every covariate",
    "separated": "the logistic null model does not converge: the covariates separate its classes",
}
SCORE_PIVOT = 2.0 ** -40
SCORE_MAX_ITER, SCORE_STEP = 50, 1e-10


def _score_cholesky(A):
    """The lower Cholesky factor of the small matrix A, or None where a pivot is <= 2^-40 of the largest diagonal
    entry (S24: collinear columns) or not finite."""
    q = A.shape[0]
    top = float(A.diagonal().max())
    L = np.zeros((q, q))
    for i in range(q):
        for j in range(i + 1):
            s = A[i, j] - float(np.dot(L[i, :j], L[j, :j]))
            if i == j:
                if not s > SCORE_PIVOT * top:
                    return None
                L[i, i] = np.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    return L


def _score_solve(L, v):
    """A^-1 v from A's lower Cholesky factor."""
    q = L.shape[0]
    u = np.zeros(q)
    for i in range(q):
        u[i] = (v[i] - np.dot(L[i, :i], u[:i])) / L[i, i]
    x = np.zeros(q)
    for i in range(q - 1, -1, -1):
        x[i] = (u[i] - np.dot(L[i + 1:, i], x[i + 1:])) / L[i, i]
    return x


def _score_null(y, X, kind):
    """The null fit of S24 on the design X [n, q]: (coef, w, r, L, mu) or the key of SCORE_SKIPS that refuses it
    (mu: the fitted values, which S25 reads)."""
    n, q = X.shape
    if kind == "linear":
        L = _score_cholesky(X.T @ X)
        if L is None:
            return "collinear"
        coef = _score_solve(L, X.T @ y)
        return coef, np.ones(n), y - X @ coef, L, X @ coef
    coef = np.zeros(q)
    with np.errstate(all="ignore"):
        converged = False
        for it in range(SCORE_MAX_ITER + 1):
            mu = 1.0 / (1.0 + np.exp(-(X @ coef)))
            w = mu * (1.0 - mu)
            r = y - mu
            L = _score_cholesky((X * w[:, None]).T @ X)
            if L is None:
                return "separated" if it else "collinear"      # at 0 every weight is 1/4: the columns themselves
            if converged:                                      # mu, w, r and L are those of the last step's end
                return coef, w, r, L, mu
            if it == SCORE_MAX_ITER:
                break
            step = _score_solve(L, X.T @ r)
            if not np.all(np.isfinite(step)):
                return "separated"
            coef = coef + step
            converged = np.max(np.abs(step)) <= SCORE_STEP
    return "separated"


def score_host(values, covariates, kind="logistic"):
    """Host side of spec S24, pure numpy: values float64 [T, N] (nan = missing; 0 / 1 for the logistic kind),
    covariates float64 [c, N] (nan = missing), 0 <= c <= 8.  Per trait the valid set (the isolates with the value
    and every covariate), the design (ones; every covariate less its mean over the valid set, divided by its largest
    absolute centred value) and the null fit: Newton steps from 0 for the logistic kind (at most 50, converged at a
    largest step <= 1e-10), least squares by the Cholesky factor of X'X for the linear one.  Returns a dict: rows
    float64 [T, q + 1, N], valid bool [T, N], chol float64 [T, q (q + 1) / 2], rss float64 [T], n int64 [T], coef
    float64 [T, q], skipped [T] (None or the key of SCORE_SKIPS that refuses the trait: its rows and valid set are
    empty, its factor is the identity), and for spec S25 mu float64 [T, N] (the fitted values of the null model) and
    design float64 [T, q, N] (the scaled design columns, row 0 ones), both zero outside the valid set."""
    if kind not in SCORE_KINDS:
        raise ValueError("score_plan: kind must be one of %s" % ", ".join(repr(k) for k in SCORE_KINDS))
    values = np.ascontiguousarray(values, dtype=np.float64)
    if values.ndim != 2:
        raise ValueError("score_plan: values must be a [T, N] array")
    T, N = values.shape
    covariates = np.zeros((0, N)) if covariates is None else np.ascontiguousarray(covariates, dtype=np.float64)
    if covariates.ndim != 2 or covariates.shape[1] != N:
        raise ValueError("score_plan: covariates must be a [c, %d] array, one row per covariate" % N)
    c = covariates.shape[0]
    if c > SCORE_MAX_COVARIATES:
        raise ValueError("score_plan: %d covariates, at most %d are taken" % (c, SCORE_MAX_COVARIATES))
    if np.isinf(values).any() or np.isinf(covariates).any():
        raise ValueError("score_plan: a value or a covariate is infinite")
    if kind == "logistic" and not np.all(np.isnan(values) | (values == 0.0) | (values == 1.0)):
        raise ValueError("score_plan: a binary trait is 0, 1 or nan")
    q = c + 1
    tri = np.tril_indices(q)
    out = dict(rows=np.zeros((T, q + 1, N)), valid=np.zeros((T, N), dtype=bool), chol=np.zeros((T, len(tri[0]))),
               rss=np.zeros(T), n=np.zeros(T, dtype=np.int64), coef=np.zeros((T, q)), skipped=[None] * T,
               mu=np.zeros((T, N)), design=np.zeros((T, q, N)))
    out["chol"][:] = np.eye(q)[tri]
    have = ~np.isnan(covariates).any(axis=0)
    for t in range(T):
        V = np.flatnonzero(~np.isnan(values[t]) & have)
        n = V.size
        fit = None
        if n <= q + 1:
            fit = "few"
        else:
            y = values[t, V]
            centred = covariates[:, V] - (np.add.accumulate(covariates[:, V], axis=1)[:, -1] / float(n))[:, None]
            scale = np.abs(centred).max(axis=1) if c else np.zeros(0)
            if c and (np.any(covariates[:, V].max(axis=1) == covariates[:, V].min(axis=1)) or not np.all(scale > 0)):
                fit = "constant"
            elif kind == "logistic" and y.min() == y.max():
                fit = "one_class"
            else:
                X = np.concatenate([np.ones((1, n)), centred / scale[:, None]]).T
                fit = _score_null(y, X, kind)
        if isinstance(fit, str):
            out["skipped"][t] = fit
            out["n"][t] = n                  # what the warning names; the plan's valid set stays empty
            continue
        coef, w, r, L, mu = fit
        out["valid"][t, V] = True
        out["n"][t] = n
        out["coef"][t] = coef
        out["rows"][t][0, V] = r
        out["rows"][t][1:, V] = (X * w[:, None]).T
        out["chol"][t] = L[tri]
        out["mu"][t, V] = mu
        out["design"][t][:, V] = X.T
        if kind == "linear":
            out["rss"][t] = np.add.accumulate(r * r)[-1] if n else 0.0          # ascending isolate order
    return out


def rank_rows(values):
    """Host ranking of spec S15, exact double comparisons: float64 [T, N] with NaN for missing -> (rc int16 [T, N],
    valid bool [T, N], n int64 [T], tiesum int64 [T], tie groups int64 [T])."""
    values = np.ascontiguousarray(values, dtype=np.float64)
    if values.ndim != 2:
        raise ValueError("ranksum_plan: values must be a [T, N] array")
    T, N = values.shape
    valid = ~np.isnan(values)
    rc = np.zeros((T, N), dtype=np.int16)
    n, tiesum, groups = (np.zeros(T, dtype=np.int64) for _ in range(3))
    for t in range(T):
        x = values[t, valid[t]]
        srt = np.sort(x)
        less = np.searchsorted(srt, x, side="left").astype(np.int64)
        equal = np.searchsorted(srt, x, side="right").astype(np.int64) - less
        n[t] = x.size
        rc[t, valid[t]] = 2 * less + equal + 1 - (x.size + 1)
        tau = np.unique(srt, return_counts=True)[1].astype(np.int64)
        tiesum[t] = int(np.sum(tau ** 3 - tau))
        groups[t] = int(np.sum(tau > 1))
    return rc, valid, n, tiesum, groups


SHIFT_MAX_ABS = 1e150          # spec S19's magnitude rule: no difference of two values overflows


class RankShiftPlan:
    """The sorted values of a rank-sum step for the Hodges-Lehmann shift (spec S19;
    AssociationEngine.ranksum_shift_plan): ``xs`` float64 [T, N] = a trait's valid values ascending in its first n
    places (zeros behind) and ``pos`` int32 [T, N] = the isolate at each sorted place, on the device; ``xs_host`` /
    ``pos_host`` the same on the host."""

    def __init__(self, xs, pos, xs_host, pos_host):
        self.xs, self.pos, self.xs_host, self.pos_host = xs, pos, xs_host, pos_host
        self.T, self.N = (int(x) for x in xs_host.shape)


def shift_rows(values):
    """Host sort of spec S19: float64 [T, N] with NaN for missing -> (xs float64 [T, N], pos int32 [T, N]); a stable
    sort, -0.0 stored as +0.0.  Raises ValueError for a value above SHIFT_MAX_ABS in magnitude."""
    values = np.ascontiguousarray(values, dtype=np.float64)
    if values.ndim != 2:
        raise ValueError("ranksum_shift_plan: values must be a [T, N] array")
    valid = ~np.isnan(values)
    if np.any(np.abs(values[valid]) > SHIFT_MAX_ABS):
        raise ValueError(shift_magnitude_text())
    xs, pos = np.zeros(values.shape, dtype=np.float64), np.zeros(values.shape, dtype=np.int32)
    for t in range(values.shape[0]):
        iso = np.flatnonzero(valid[t])
        x = values[t, iso] + 0.0
        order = np.argsort(x, kind="stable")
        xs[t, :iso.size], pos[t, :iso.size] = x[order], iso[order]
    return xs, pos


def shift_magnitude_text():
    return ("the Hodges-Lehmann shift takes values up to 1e150 in magnitude: beyond it a difference of two values "
            "could overflow")


class VanElterenPlan:
    """The quantitative traits of a stratified rank-sum step (spec S16; AssociationEngine.vanelteren_plan).  On the
    device: ``score`` int16 [T, N] = w_s Rc_i with Rc the centred doubled midrank inside the stratum (0 where the
    value is missing), ``l`` int16 [T, N] = the scores of the valid isolates by (stratum, isolate), ``valid`` the
    validity rows (vecrows, int32 [T, Wp]), ``wn`` int32 [T, S, 2] = (w_s, n_s), ``c`` float64 [T, S], ``strata``
    int16 [N] (uint16 bit pattern) and ``members`` int32 [N].  On the host: score_host, valid_host (bool [T, N]),
    strata_host int64 [N], w, n, tiesum, tie_groups int64 [T, S] and c_host float64 [T, S]."""

    def __init__(self, dev, score_host, valid_host, strata_host, S, w, n, tiesum, tie_groups, c_host):
        self.score, self.l, self.valid, self.wn, self.c, self.strata, self.members = dev
        self.score_host, self.valid_host, self.strata_host = score_host, valid_host, strata_host
        self.w, self.n, self.tiesum, self.tie_groups, self.c_host = w, n, tiesum, tie_groups, c_host
        self.S = int(S)
        self.T, self.N = (int(x) for x in score_host.shape)


VANELTEREN_MAX_SCORE = 16319                      # |w_s Rc_i| <= 16319: the hi digit of S15's split fits a signed byte


def vanelteren_rows(values, strata, S):
    """Host ranking of spec S16, exact double comparisons: float64 [T, N] with NaN for missing and the stratum of
    every isolate -> (score int16 [T, N], l int16 [T, N], valid bool [T, N], w, n, tiesum, tie groups int64 [T, S],
    c float64 [T, S])."""
    values = np.ascontiguousarray(values, dtype=np.float64)
    if values.ndim != 2:
        raise ValueError("vanelteren_plan: values must be a [T, N] array")
    T, N = values.shape
    valid = ~np.isnan(values)
    score, l = np.zeros((T, N), dtype=np.int16), np.zeros((T, N), dtype=np.int16)
    w, n, tiesum, groups = (np.zeros((T, S), dtype=np.int64) for _ in range(4))
    c = np.zeros((T, S), dtype=np.float64)
    members = [np.flatnonzero(strata == s) for s in range(S)]
    for t in range(T):
        k = 0
        for s in range(S):
            who = members[s][valid[t, members[s]]]
            ns = who.size
            if ns == 0:
                continue
            rc, _valid, _n, ts, gr = rank_rows(values[t:t + 1, who])
            ws = max(1, VANELTEREN_MAX_SCORE // (ns + 1))
            score[t, who] = ws * rc[0].astype(np.int64)
            l[t, k:k + ns] = score[t, who]
            k += ns
            w[t, s], n[t, s], tiesum[t, s], groups[t, s] = ws, ns, ts[0], gr[0]
            if ns >= 2:
                f = float(ns + 1) - float(ts[0]) / (float(ns) * float(ns - 1))
                c[t, s] = float(ws * ws) * f / 12.0
    return score, l, valid, w, n, tiesum, groups, c


class Workspace:
    """Device buffers of one associate() step (engine.workspace)."""

    def __init__(self, eng, genes, T, permutations, use_lists, perm_buffer=None):
        torch = _torch()
        G, N = genes.G, genes.N
        self.key = (G, N, int(T), int(permutations), bool(use_lists and permutations > 0))
        self.eng = eng
        self.counts = eng._empty((T, G, 4), torch.int32)
        self.margins = eng._empty((T, 2), torch.int32)
        self.mask_class = eng._empty((T,), torch.int32)
        self.plan_buf = eng._empty((int(eng.lib.scoary_trait_plan_bytes(int(T), N)) // 4,), torch.int32)
        self.p = eng._empty((T, G), torch.float64)
        self.odds = eng._empty((T, G), torch.float64)
        self.crit = eng._empty((T, G, 2), torch.int32) if permutations > 0 else None
        self.r = eng._empty((T, G), torch.int32) if permutations > 0 else None
        self.tiles = self.scratch = self.perms = self.lcrit = self.bfrag = None
        self.label_shards = None
        self.auto = None        # engine.associate's cached hipGraph of a launch-bound step
        self.batch = 0
        if permutations > 0 and use_lists:
            self.batch = eng.list_batch(T, N, permutations, G)
            nb0 = min(self.batch, permutations)
            words = int(eng.lib.scoary_list_tiles_words(N, nb0, T))
            if eng.label_shards is not None:          # room for world equal chunks (dist.LabelShards)
                words = max(words, eng.label_shards.padded_words(*eng.tiles_per_batch(N, nb0, T)))
            self.tiles = eng._empty((words,), torch.int32)
            self.label_shards = eng.label_shards
            self.scratch = eng.permute_lists_scratch(G, T, N, nb0)
            self.lcrit = eng._empty((T, G, 2), torch.int32)
            eng.fisher_chains(T, N)           # the Fisher pass's slabs: allocated here, not inside a captured step
            # B operand of the matrix-core kernel, one label batch
            if genes.lists is not None and genes.lists.panels is not None:
                self.bfrag = eng._empty((int(eng.lib.scoary_mfma_bfrag_bytes(N, nb0, T)) // 4,), torch.int32)
        elif permutations > 0:
            if perm_buffer is not None:
                self.perms = perm_buffer
            else:
                self.perms = eng._empty((T, eng.perm_batch(T, N, permutations), eng.row_words(N)),
                                        torch.int32)

    def fits(self, genes, T, permutations, use_lists):
        # the label shards are part of the shape: a workspace made before eng.label_shards was set
        # (or kept after it was reset) has the wrong tile padding, and ranks that disagree about
        # the shards would block in the all-gather of _label_tiles
        if self.tiles is not None and self.label_shards is not self.eng.label_shards:
            return False
        return self.key == (genes.G, genes.N, int(T), int(permutations),
                            bool(use_lists and permutations > 0))


class StepGraph:
    """A captured associate() step (engine.capture)."""

    def __init__(self, eng, graph, stream):
        self.eng, self.graph, self.stream = eng, graph, stream
        self.done = None        # event behind the most recent launch

    def launch(self):
        eng = self.eng
        eng._check(eng.lib.scoary_graph_launch(eng.h, self.graph, eng._stream()),
                   "scoary_graph_launch")
        if self.done is None:
            self.done = _torch().cuda.Event()
        self.done.record(_torch().cuda.current_stream(eng.device))

    def close(self):
        """Destroys the executable graph -- after its last launch has finished: the runtime
        does not keep a destroyed graph alive for a launch that is still running."""
        if self.graph:
            if self.done is not None:
                self.done.synchronize()
            self.eng.lib.scoary_graph_destroy(self.graph)
            self.graph = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AssociationEngine:
    def __init__(self, device=None):
        torch = _torch()
        if not torch.cuda.is_available():
            raise _abi.ScoaryHipError(
                "no GPU visible: scoary_amd runs on MI355X (gfx950) only and has no CPU path")
        self.lib = _abi.load()
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", int(device) if not isinstance(device, torch.device)
                                   else device.index or 0)
        h = ctypes.c_void_p()
        rc = self.lib.scoary_create(self.device.index, ctypes.byref(h))
        if rc != 0:
            raise _abi.ScoaryHipError("scoary_create(device=%d) failed: %d" % (self.device.index, rc))
        self.h = h
        # dist.LabelShards: generate one share of every batch of label tiles and all-gather the
        # rest (multi-GPU, opt-in); None: every rank generates all tiles (the default)
        self.label_shards = None
        # the label generator writes the matrix-core kernel's B fragments next to its tiles (_label_tiles);
        # False: the tiles alone, and every permute_lists converts them (k_mfma_bfrag) -- for comparisons
        self.fuse_bfrag = True

    def close(self):
        if getattr(self, "h", None):
            self.lib.scoary_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- plumbing -----------------------------------------------------------
    def _side_stream(self):
        if getattr(self, "_side", None) is None:
            self._side = _torch().cuda.Stream(device=self.device)
        return self._side

    def _stream(self):
        return ctypes.c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.scoary_last_error(self.h)
            raise _abi.ScoaryHipError("%s failed (%d): %s" % (what, rc, (msg or b"").decode()))

    @staticmethod
    def _ptr(t):
        return ctypes.c_void_p(t.data_ptr())

    def quads(self, N):
        return int(self.lib.scoary_tiled_quads(int(N)))

    def row_words(self, N):
        return int(self.lib.scoary_row_words(int(N)))

    def padded_genes(self, G):
        return int(self.lib.scoary_tiled_genes(int(G)))

    def _empty(self, shape, dtype):
        return _torch().empty(shape, dtype=dtype, device=self.device)

    # -- a1: packing ----------------------------------------------------------
    def pack_dense(self, dense):
        """dense: (G, N) uint8 (numpy or device tensor), non-zero = present."""
        torch = _torch()
        if isinstance(dense, np.ndarray):
            dense = torch.from_numpy(np.ascontiguousarray(dense, dtype=np.uint8))
        dense = dense.to(self.device, dtype=torch.uint8).contiguous()
        G, N = dense.shape
        tiled = self._empty((self.quads(N), self.padded_genes(G), 4), torch.int32)
        self._check(self.lib.scoary_pack_dense(self.h, self._ptr(dense), G, N, self._ptr(tiled),
                                               self._stream()), "scoary_pack_dense")
        return GeneMatrix(tiled, G, N)

    def tile_rows(self, rows64, N):
        """rows64: (G, W64) uint64 bit rows (numpy or int64 device tensor)."""
        torch = _torch()
        if isinstance(rows64, np.ndarray):
            rows64 = torch.from_numpy(np.ascontiguousarray(rows64).view(np.int64))
        rows64 = rows64.to(self.device).contiguous()
        G, W = rows64.shape
        if W != (N + 63) // 64:
            raise ValueError("rows64 has %d words per row, N=%d needs %d" % (W, N, (N + 63) // 64))
        tiled = self._empty((self.quads(N), self.padded_genes(G), 4), torch.int32)
        self._check(self.lib.scoary_tile_rows(self.h, self._ptr(rows64), G, N, self._ptr(tiled),
                                              self._stream()), "scoary_tile_rows")
        return GeneMatrix(tiled, G, N)

    def vecrows(self, rows64, N):
        """(R, W64) uint64 host rows -> device vecrows int32 [R, Wp] (zero padded)."""
        torch = _torch()
        rows64 = np.ascontiguousarray(rows64, dtype=np.uint64)
        R, W = rows64.shape
        Wp = self.row_words(N)
        buf = np.zeros((R, Wp), dtype=np.uint32)
        buf[:, :2 * W] = rows64.view(np.uint32).reshape(R, 2 * W)
        return torch.from_numpy(buf.view(np.int32)).to(self.device)

    def list_budget_bytes(self):
        """Bytes build_lists may spend on one matrix's index array: SCOARY_LIST_BUDGET_MB if set
        (tests), else 60 % of the device memory that is free right now (the driver's figure plus what
        torch's caching allocator holds unused) -- label tiles (<= 8 GB)
        and the count scratch (<= 4 GB) of a step still have to fit next to it."""
        import os
        mb = os.environ.get("SCOARY_LIST_BUDGET_MB")
        if mb:
            return int(float(mb) * (1 << 20))
        torch = _torch()
        free, _total = torch.cuda.mem_get_info(self.device)
        # blocks the caching allocator holds but has not handed out are as good as free
        cached = torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
        return int((free + max(cached, 0)) * 0.6)

    def list_kernel_name(self, N):
        """Timer label (scoary_last_kernel_ms) of the list-driven permutation kernel that
        takes N isolates: k_permute_lists (one tile in LDS) or k_permute_seglists (N > 20479)."""
        return "k_permute_seglists" if int(self.lib.scoary_list_segments(int(N))) > 1 else "k_permute_lists"

    def build_lists(self, genes, budget_bytes=None):
        """Attach the minority index lists of ``genes`` (spec S6) for the list-driven
        permutation kernel.  Built on the device from the tiled matrix that is
        already in HBM (scoary_lists_plan + scoary_lists_fill): nothing crosses
        PCIe but the 8-byte entry count.  The plan returns the size of the index array
        before it is allocated: more than ``budget_bytes`` (default list_budget_bytes())
        raises ListMemoryError and leaves ``genes.lists`` None."""
        torch = _torch()
        lanes, _stride, _gpw, _classes, _piece = self.list_params(genes.N)
        if not lanes:
            raise ValueError("N=%d is too large for the list-driven kernel" % genes.N)
        G, N = genes.G, genes.N
        scratch = self._empty((int(self.lib.scoary_lists_scratch_bytes(G, N)) // 8 + 1,),
                              torch.int64)
        nseg = max(1, int(self.lib.scoary_list_segments(N)))      # N > 20479: sub-lists per segment
        shape = (G,) if nseg == 1 else (nseg, G)
        start = self._empty(shape, torch.int32)
        ngroups = self._empty(shape, torch.int32)
        order = self._empty((G,), torch.int32)
        flipped = self._empty((G,), torch.uint8)
        entries = ctypes.c_int64()
        self._check(self.lib.scoary_lists_plan(
            self.h, self._ptr(genes.tiled), G, N, self._ptr(scratch), self._ptr(start),
            self._ptr(ngroups), self._ptr(order), self._ptr(flipped), ctypes.byref(entries),
            self._stream()), "scoary_lists_plan")
        total = int(entries.value)                     # 32-bit words of index array
        need = 4 * (total + int(self.lib.scoary_lists_slack_entries()))
        if budget_bytes is None:
            budget_bytes = self.list_budget_bytes()
        if need > budget_bytes:
            raise ListMemoryError("index lists of a %d x %d matrix need %.1f MB, budget %.1f MB"
                                  % (G, N, need / 2**20, budget_bytes / 2**20))
        idx = self._empty((total + int(self.lib.scoary_lists_slack_entries()),), torch.int32)
        self._check(self.lib.scoary_lists_fill(
            self.h, self._ptr(genes.tiled), G, N, self._ptr(scratch), self._ptr(order),
            self._ptr(flipped), total, self._ptr(idx), self._stream()), "scoary_lists_fill")
        genes.lists = GeneLists(idx, start, ngroups, order, flipped, total, N)
        self._build_panels(genes, budget_bytes - need)
        return genes.lists

    def _build_panels(self, genes, budget_bytes):
        """The matrix-core operands of the list slots (N <= 2048, 1 KB per slot; skipped when they do
        not fit the budget: the lists then take every gene) and what the routing needs on the host."""
        torch = _torch()
        L, G, N = genes.lists, genes.G, genes.N
        nbytes = int(self.lib.scoary_mfma_panels_bytes(G, N))
        if nbytes == 0 or nbytes > budget_bytes:
            return
        panels = self._empty((nbytes // 4,), torch.int32)
        self._check(self.lib.scoary_mfma_panels_build(
            self.h, self._ptr(genes.tiled), G, N, self._ptr(L.order), self._ptr(L.flipped),
            self._ptr(panels), self._stream()), "scoary_mfma_panels_build")
        starts = L.start[::256].to(torch.int64).cpu().numpy() * 32    # d_lstart counts units of 32 entries
        L.block_start = np.ascontiguousarray(np.append(starts, np.int64(L.entries)), dtype=np.int64)
        L.panels = panels

    def mfma_split(self, genes, T, P):
        """Slots [0, k_split) of a (T, P) launch go to the matrix-core kernel: scoary_mfma_route (the
        handle's routing mode, the two measured rates, the launch shape), cached per data set."""
        L = genes.lists
        if L is None or L.panels is None:
            return 0
        key = (getattr(self, "_mfma_mode", "auto"), int(T), int(P))
        k = L.routes.get(key)
        if k is None:
            k = L.routes[key] = int(self.lib.scoary_mfma_route(
                self.h, ctypes.c_void_p(L.block_start.ctypes.data), genes.G, int(T), genes.N, int(P)))
        return k

    def set_mfma_route(self, mode):
        """Which list slots the matrix-core kernel takes: "none", "all" or "auto" (the default: the slots
        above the measured break-even list length) -- scoary_set_mfma_route."""
        self._check(self.lib.scoary_set_mfma_route(self.h, {"none": 0, "all": 1, "auto": 2}[mode]),
                    "scoary_set_mfma_route")
        self._mfma_mode = mode

    def list_params(self, N):
        """(tile row dwords, row stride bytes, genes per wavefront, classes,
        interleave piece) -- scoary_list_params."""
        out = (ctypes.c_int64 * 5)()
        self.lib.scoary_list_params(int(N), out)
        return tuple(int(x) for x in out)

    def lists_supported(self, N):
        return int(N) <= int(self.lib.scoary_list_max_isolates())

    def perm_generate_tiles(self, masks, margins, N, P, perm_base, seed, out=None, trait_base=0,
                            tile_range=None, strata=None, bfrag=None):
        """Label tiles of permutations perm_base .. perm_base + P - 1 (perm_base a multiple of
        32).  ``tile_range`` = (first, count): only these flat (trait, tile) indices of the
        [T][tiles] array are written (scoary_perm_generate_tiles_range) -- one rank's share of a
        run that all-gathers the rest (dist.LabelShards).  ``strata``: a StrataPlan of these traits --
        the labels are shuffled within its strata (spec S9).  ``bfrag``: a buffer of scoary_mfma_bfrag_bytes(N, P, T)
        bytes that also takes the B fragments of the written tiles' stages (N <= 2048), ready for
        permute_lists(..., bfrag=bfrag, bfrag_ready=True)."""
        torch = _torch()
        T = masks.shape[0]
        if out is None:
            out = self._empty((int(self.lib.scoary_list_tiles_words(N, P, T)),), torch.int32)
        if bfrag is not None:
            if tile_range is None:
                tile_range = (0, self.tiles_per_batch(N, P, T)[0])
            if strata is not None:
                self._strata_fits(strata, T, N)
                self._check(self.lib.scoary_perm_generate_tiles_strata_bfrag_range(
                    self.h, self._ptr(masks), *self._strata_ptrs(strata), T, N, strata.S, P, perm_base, trait_base,
                    ctypes.c_uint64(seed), int(tile_range[0]), int(tile_range[1]), self._ptr(out), self._ptr(bfrag),
                    self._stream()), "scoary_perm_generate_tiles_strata_bfrag_range")
            else:
                self._check(self.lib.scoary_perm_generate_tiles_bfrag_range(
                    self.h, self._ptr(masks), self._ptr(margins), T, N, P, perm_base, trait_base,
                    ctypes.c_uint64(seed), int(tile_range[0]), int(tile_range[1]), self._ptr(out), self._ptr(bfrag),
                    self._stream()), "scoary_perm_generate_tiles_bfrag_range")
        elif strata is not None:
            self._strata_fits(strata, T, N)
            if tile_range is None:
                tile_range = (0, self.tiles_per_batch(N, P, T)[0])
            self._check(self.lib.scoary_perm_generate_tiles_strata_range(
                self.h, self._ptr(masks), *self._strata_ptrs(strata), T, N, strata.S, P, perm_base, trait_base,
                ctypes.c_uint64(seed), int(tile_range[0]), int(tile_range[1]), self._ptr(out), self._stream()),
                "scoary_perm_generate_tiles_strata_range")
        elif tile_range is None:
            self._check(self.lib.scoary_perm_generate_tiles(
                self.h, self._ptr(masks), self._ptr(margins), T, N, P, perm_base, trait_base,
                ctypes.c_uint64(seed), self._ptr(out), self._stream()), "scoary_perm_generate_tiles")
        else:
            self._check(self.lib.scoary_perm_generate_tiles_range(
                self.h, self._ptr(masks), self._ptr(margins), T, N, P, perm_base, trait_base,
                ctypes.c_uint64(seed), int(tile_range[0]), int(tile_range[1]), self._ptr(out),
                self._stream()), "scoary_perm_generate_tiles_range")
        return out

    def tiles_per_batch(self, N, P, T):
        """Flat (trait, tile) count and dwords per tile of a batch of P permutations."""
        tw = self.list_params(N)[0]
        return int(T) * (-(-int(P) // (32 * tw))), int(self.lib.scoary_list_tile_words(int(N)))

    def permute_lists_scratch(self, G, T, N, P):
        """Scratch tensor for permute_lists (list-order regions + per-part counts)."""
        torch = _torch()
        nbytes = int(self.lib.scoary_permute_lists_scratch_bytes(G, T, N, P))
        return self._empty(((nbytes + 3) // 4,), torch.int32)

    def permute_lists(self, genes, tiles, crit, margins, P, r, scratch=None, lcrit=None,
                      accumulate=True, bfrag=None, bfrag_ready=False):
        """r (+)= exceedance counts of P permutations (label tiles ``tiles``).  The regions
        come in gene order (``crit`` from fisher) or, one launch cheaper, in slot order
        (``lcrit`` from fisher(..., lists=...)); accumulate=False overwrites r.  ``bfrag_ready``: ``bfrag`` already
        holds the B fragments of ``tiles`` (perm_generate_tiles(..., bfrag=bfrag) of the same N, P, T)."""
        L = genes.lists
        T = (lcrit if lcrit is not None else crit).shape[0]
        if scratch is None:
            scratch = self.permute_lists_scratch(genes.G, T, genes.N, P)
        # the long-list slots [0, k_split) go to the matrix-core kernel (a host-side decision: the
        # handle's routing mode, the data set's break-even count and the launch shape)
        routed = 0
        k_split = self.mfma_split(genes, T, P)
        if k_split > 0:
            if bfrag is None:
                bfrag = self._empty((int(self.lib.scoary_mfma_bfrag_bytes(genes.N, P, T)) // 4,), _torch().int32)
            routed = int(L.block_start[-1 if k_split >= genes.G else k_split // 256])
        self._check(self.lib.scoary_permute_hybrid_bfrag(
            self.h, self._ptr(tiles), self._ptr(L.idx), L.entries, self._ptr(L.start),
            self._ptr(L.ngroups), self._ptr(L.order), self._ptr(L.flipped),
            self._ptr(crit) if lcrit is None else None,
            self._ptr(lcrit) if lcrit is not None else None,
            self._ptr(margins), self._ptr(scratch), genes.G, T, genes.N, P, self._ptr(r),
            1 if accumulate else 0, self._ptr(L.panels) if k_split > 0 else None,
            self._ptr(bfrag) if k_split > 0 else None, k_split, routed, 1 if bfrag_ready and k_split > 0 else 0,
            self._stream()), "scoary_permute_hybrid_bfrag")
        return r

    # -- a3: counts -----------------------------------------------------------
    def trait_plan(self, traits, masks, N, out=None):
        """Margins, mask classes and the gathered operand rows of a trait set (scoary_trait_plan),
        once per trait set.  ``out`` = (margins, mask_class, plan buffer) to fill."""
        torch = _torch()
        T = traits.shape[0]
        margins, mask_class, buf = out if out is not None else (
            self._empty((T, 2), torch.int32), self._empty((T,), torch.int32),
            self._empty((int(self.lib.scoary_trait_plan_bytes(int(T), int(N))) // 4,), torch.int32))
        self._check(self.lib.scoary_trait_plan(self.h, self._ptr(traits), self._ptr(masks), T, int(N),
                                               self._ptr(margins), self._ptr(mask_class), self._ptr(buf),
                                               self._stream()), "scoary_trait_plan")
        return TraitPlan(margins, mask_class, buf, traits, masks, N)

    def counts(self, genes, traits, masks, out=None, plan=None):
        """-> (counts int32 [T, G, 4], margins int32 [T, 2]).  ``plan``: the TraitPlan of these
        traits / masks (trait_plan); without one it is built here (three more small launches).
        ``out`` = (counts[, margins, mask_class, plan buffer]): buffers to fill."""
        torch = _torch()
        T = traits.shape[0]
        counts = out[0] if out is not None else self._empty((T, genes.G, 4), torch.int32)
        if plan is None:
            plan = self.trait_plan(traits, masks, genes.N,
                                   out=None if out is None or len(out) < 4 else tuple(out[1:4]))
        elif not plan.fits(traits, masks) or plan.N != genes.N:
            raise ValueError("the trait plan was built from other trait / mask tensors")
        self._check(self.lib.scoary_counts_planned(
            self.h, self._ptr(genes.tiled), self._ptr(plan.buf), self._ptr(plan.margins),
            genes.G, T, genes.N, self._ptr(counts), self._stream()), "scoary_counts_planned")
        return counts, plan.margins

    # -- a5: Fisher -----------------------------------------------------------
    def fisher(self, tables, want_crit=True, out=None, lists=None, lcrit=None):
        """tables: int32 device tensor [..., 4] -> (p, odds, crit) shaped [...].
        With ``lists`` (the GeneLists of the matrix the [T, G, 4] tables were counted on):
        scoary_fisher_lists -- tables visited in list-slot order, and the regions also
        written in the list kernel's form; returns (p, odds, crit, lcrit).  Where the weight chains of the
        tables' margin classes fit their budget (fisher_chains) the pass is scoary_fisher_lists_chained: the same
        bits from two kernels that divide once per class, not once per table, for launches large enough to pay
        for the chain kernel (set_fisher_route)."""
        torch = _torch()
        tables = tables.contiguous()
        shape = tables.shape[:-1]
        M = int(np.prod(shape)) if len(shape) else 1
        if out is not None:
            p, odds, crit = out
        else:
            p = self._empty(shape, torch.float64)
            odds = self._empty(shape, torch.float64)
            crit = self._empty(tuple(shape) + (2,), torch.int32) if want_crit else None
        if lists is not None:
            if len(shape) != 2:
                raise ValueError("fisher(lists=...) wants tables shaped [T, G, 4]")
            if lcrit is None:
                lcrit = self._empty(tuple(shape) + (2,), torch.int32)
            chains = self.fisher_chains(shape[0], lists.N)
            self._check(self.lib.scoary_fisher_lists_chained(
                self.h, self._ptr(tables), shape[0], shape[1], lists.N, self._ptr(lists.order),
                self._ptr(lists.flipped), self._ptr(p), self._ptr(odds),
                self._ptr(crit) if crit is not None else None, self._ptr(lcrit),
                self._ptr(chains) if chains is not None else None,
                chains.numel() * 4 if chains is not None else 0, self._stream()), "scoary_fisher_lists_chained")
            return p, odds, crit, lcrit
        self._check(self.lib.scoary_fisher(self.h, self._ptr(tables), M, self._ptr(p),
                                           self._ptr(odds),
                                           self._ptr(crit) if crit is not None else None,
                                           self._stream()), "scoary_fisher")
        return p, odds, crit

    def fisher_chains(self, T, N):
        """The scratch of scoary_fisher_lists_chained for T traits of an N-isolate matrix (None: the slabs exceed
        the library's budget and the pass runs the one-kernel walk).  Cached on the engine by size and rewritten
        by every pass; never replaced, because a captured step holds its address.  A capture must find it there
        (a Workspace allocates it)."""
        torch = _torch()
        need = int(self.lib.scoary_fisher_chains_bytes(int(T), int(N)))
        if need == 0:
            return None
        cache = self.__dict__.setdefault("_fisher_chains", {})
        buf = cache.get(need)
        if buf is None:
            if torch.cuda.is_current_stream_capturing():
                raise ValueError("fisher(lists=...) inside a graph capture needs its chain slabs allocated before "
                                 "the capture: make the step's Workspace (or call fisher_chains(T, N)) first")
            buf = cache[need] = self._empty((need // 4,), torch.int32)
        return buf

    def set_fisher_route(self, mode):
        """The kernels of fisher(lists=...): "walk" (every table walks its own weights: the kernel of
        scoary_fisher_lists), "chains" (one weight chain per margin class, whenever the slabs fit) or "auto" (the
        default: the chains for launches large enough to pay for the chain kernel) -- scoary_set_fisher_route."""
        self._check(self.lib.scoary_set_fisher_route(self.h, {"walk": 0, "chains": 1, "auto": 2}[mode]),
                    "scoary_set_fisher_route")

    def fisher_scipy(self, tables, p):
        """SciPy's own double for every table of 171 ... fisher_scipy_max_isolates() isolates, written over the
        entries of ``p`` (float64 device tensor shaped like tables[..., 0]; scoary_fisher_scipy): what the command
        line prints.  Returns the number of tables above the maximum (left as they were)."""
        torch = _torch()
        tables = tables.contiguous()
        if not p.is_contiguous() or p.dtype != torch.float64 or tuple(p.shape) != tuple(tables.shape[:-1]):
            raise ValueError("fisher_scipy: p must be a contiguous float64 tensor shaped like the tables")
        M = int(np.prod(tables.shape[:-1])) if len(tables.shape) > 1 else 1
        skipped = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._check(self.lib.scoary_fisher_scipy(self.h, self._ptr(tables), M, self._ptr(p), self._ptr(skipped),
                                                 self._stream()), "scoary_fisher_scipy")
        return int(skipped.item())

    def fisher_scipy_max_isolates(self):
        return int(self.lib.scoary_fisher_scipy_max_isolates())

    # -- a8 / a7: permutations -------------------------------------------------
    def strata_max(self):
        """(most strata, most isolates) the stratified label generator takes."""
        return int(self.lib.scoary_perm_max_strata()), int(self.lib.scoary_perm_strata_max_isolates())

    def strata_plan(self, strata_host, trait_rows, mask_rows, N, S=None):
        """The StrataPlan of ``strata_host`` (N integers in [0, S); S = the largest + 1 unless given) for the
        label rows ``trait_rows`` and validity rows ``mask_rows`` (vecrows [T, Wp], as trait_plan takes them).
        Members and offsets are built on the host (StrataPlan checks a host copy of them, also for a plan put
        together by hand: the library takes them as device arrays), the per-stratum margins by k_strata_margins."""
        torch = _torch()
        N = int(N)
        st = np.asarray(strata_host)
        if st.ndim != 1 or st.shape[0] != N or N < 1 or not np.issubdtype(st.dtype, np.integer):
            raise ValueError("strata_plan: strata must be %d integers, one per isolate" % N)
        st = st.astype(np.int64)
        S = int(st.max()) + 1 if S is None else int(S)
        max_s, max_n = self.strata_max()
        if st.min() < 0 or st.max() >= S:
            raise ValueError("strata_plan: stratum indices must lie in [0, S)")
        if S > max_s:
            raise ValueError("strata_plan: %d strata, the generator takes %d (scoary_perm_max_strata)" % (S, max_s))
        if N > max_n:
            raise ValueError("strata_plan: %d isolates, the stratified generator takes %d "
                             "(scoary_perm_strata_max_isolates)" % (N, max_n))
        sizes = np.bincount(st, minlength=S)
        members = np.argsort(st, kind="stable").astype(np.int32)
        offsets = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
        T = int(trait_rows.shape[0])
        dev = [torch.from_numpy(x).to(self.device) for x in
               (st.astype(np.uint16).view(np.int16), members, offsets)]
        smargins = self._empty((T, S, 2), torch.int32)
        self._check(self.lib.scoary_strata_margins(self.h, self._ptr(trait_rows), self._ptr(mask_rows),
                                                   self._ptr(dev[0]), T, N, S, self._ptr(smargins),
                                                   self._stream()), "scoary_strata_margins")
        return StrataPlan(dev[0], dev[1], dev[2], smargins, S, N, sizes)

    @staticmethod
    def _strata_fits(strata, T, N):
        if strata.T != int(T) or strata.N != int(N) or not strata.smargins.is_contiguous():
            raise ValueError("the strata plan was built for other traits (%d traits, %d isolates)"
                             % (strata.T, strata.N))

    def _strata_ptrs(self, strata):
        """The four device arrays of a StrataPlan, in the order the stratified generators take them."""
        return tuple(self._ptr(x) for x in (strata.strata, strata.members, strata.offsets, strata.smargins))

    # -- Cochran-Mantel-Haenszel test over the strata (spec S10) -------------------
    def _cmh_scratch(self, N):
        """The buffer of the segment table that scoary_cmh, scoary_cmh_minp_plan and scoary_cmh_exact build."""
        return self._empty(((int(self.lib.scoary_cmh_scratch_bytes(N)) + 7) // 8,), _torch().int64)

    def cmh(self, genes, traits, masks, strata, scounts=False):
        """The stratified test of every (trait, gene) over the strata of ``strata`` (the StrataPlan of these label
        rows ``traits`` and validity rows ``masks``): dict of device tensors -- stat (the continuity-corrected CMH
        chi-square, nan without an informative stratum), p, odds (the Mantel-Haenszel common odds ratio), e2 (twice
        the expectation of the pooled count) and var, float64 [T, G]; a int32 [T, G] = the pooled count
        popc(gene & label); crit int32 [T, G, 2] (uint32 bits) = the rejection region of the pooled count under
        within-stratum shuffles, in the form permute() / permute_lists(crit=...) take.  ``scounts=True`` adds
        scounts int32 [T, G, S, 2] = (a, m) of every stratum (tests; T G S 8 bytes)."""
        torch = _torch()
        T, G, N = int(traits.shape[0]), genes.G, genes.N
        self._strata_fits(strata, T, N)
        if int(masks.shape[0]) != T or not (traits.is_contiguous() and masks.is_contiguous()):
            raise ValueError("cmh: label and validity rows must be contiguous [T, Wp] tensors of the same traits")
        out = {k: self._empty((T, G), torch.float64) for k in ("stat", "p", "odds", "e2", "var")}
        out["a"] = self._empty((T, G), torch.int32)
        out["crit"] = self._empty((T, G, 2), torch.int32)
        if scounts:
            out["scounts"] = self._empty((T, G, strata.S, 2), torch.int32)
        scratch = self._cmh_scratch(N)
        self._check(self.lib.scoary_cmh(
            self.h, self._ptr(genes.tiled), self._ptr(traits), self._ptr(masks), *self._strata_ptrs(strata),
            G, T, N, strata.S, *(self._ptr(out[k]) for k in ("stat", "p", "odds", "e2", "var", "a", "crit")),
            self._ptr(out["scounts"]) if scounts else None, self._ptr(scratch), self._stream()), "scoary_cmh")
        return out

    def cmh_homogeneity(self, genes, traits, masks, strata, cmh_res):
        """The Breslow-Day test of homogeneity of the odds ratios over the strata of ``strata``, with Tarone's
        correction (spec S14; scoary_cmh_homogeneity): the test of the assumption cmh() makes, one common odds ratio.
        ``traits`` / ``masks`` / ``strata``: as cmh() takes them; ``cmh_res``: cmh()'s result for them (its odds is
        read, never recomputed: the fitted tables belong to the odds ratio that is reported).  Dict of device tensors:
        stat_bd, stat_tarone and p (the chi-square upper tail of stat_tarone) float64 [T, G], df int32 [T, G] = the
        informative strata less one.  Without a finite positive odds ratio or with fewer than two informative
        strata: (nan, nan, 1, df 0)."""
        torch = _torch()
        T, G, N = int(traits.shape[0]), genes.G, genes.N
        self._strata_fits(strata, T, N)
        if int(masks.shape[0]) != T or not (traits.is_contiguous() and masks.is_contiguous()):
            raise ValueError("cmh_homogeneity: label and validity rows must be contiguous [T, Wp] tensors of the "
                             "same traits")
        odds = cmh_res["odds"]
        if not odds.is_contiguous() or tuple(odds.shape) != (T, G) or odds.dtype != torch.float64:
            raise ValueError("cmh_homogeneity: cmh()'s odds [T, G] of the same traits, contiguous")
        out = {k: self._empty((T, G), torch.float64) for k in ("stat_bd", "stat_tarone", "p")}
        out["df"] = self._empty((T, G), torch.int32)
        scratch = self._cmh_scratch(N)
        self._check(self.lib.scoary_cmh_homogeneity(
            self.h, self._ptr(genes.tiled), self._ptr(traits), self._ptr(masks), *self._strata_ptrs(strata),
            G, T, N, strata.S, self._ptr(odds), *(self._ptr(out[k]) for k in ("stat_bd", "stat_tarone", "df", "p")),
            self._ptr(scratch), self._stream()), "scoary_cmh_homogeneity")
        return out

    def perm_generate(self, masks, margins, N, P, perm_base, seed, out=None, trait_base=0, strata=None):
        """Label rows [T, P, Wp] of the permutations perm_base .. perm_base + P - 1 (spec S4); with ``strata``
        (a StrataPlan of these traits) shuffled within its strata (spec S9)."""
        torch = _torch()
        T = masks.shape[0]
        Wp = self.row_words(N)
        if out is None:
            out = self._empty((T, P, Wp), torch.int32)
        if strata is not None:
            self._strata_fits(strata, T, N)
            self._check(self.lib.scoary_perm_generate_strata(
                self.h, self._ptr(masks), *self._strata_ptrs(strata), T, N, strata.S, P, perm_base, trait_base,
                ctypes.c_uint64(seed), self._ptr(out), self._stream()), "scoary_perm_generate_strata")
            return out
        self._check(self.lib.scoary_perm_generate(self.h, self._ptr(masks), self._ptr(margins), T,
                                                  N, P, perm_base, trait_base,
                                                  ctypes.c_uint64(seed),
                                                  self._ptr(out), self._stream()),
                    "scoary_perm_generate")
        return out

    def permute(self, genes, perms, crit, r, P=None):
        T = perms.shape[0]
        if P is None:
            P = perms.shape[1]
        self._check(self.lib.scoary_permute(self.h, self._ptr(genes.tiled), self._ptr(perms),
                                            self._ptr(crit), genes.G, T, genes.N, P,
                                            self._ptr(r), self._stream()), "scoary_permute")
        return r

    def permute_sequential(self, genes, masks, margins, crit, permutations, seed, thr, strata=None):
        """The reference's sequential estimator with early abort on the Fisher statistic
        (scoary_permute_seq): returns (r, nstop) int32 device tensors [T, G]; Empirical_p =
        (r + 1) / ((nstop or P) + 1).  ``thr``: host array of abort thresholds per
        permutation index (tree._abort_thresholds).  ``strata``: a StrataPlan (labels of spec S9)."""
        torch = _torch()
        T = masks.shape[0]
        r = torch.zeros((T, genes.G), dtype=torch.int32, device=self.device)
        nstop = torch.zeros((T, genes.G), dtype=torch.int32, device=self.device)
        th = np.minimum(np.asarray(thr, dtype=np.int64), 0xffffffff).astype(np.uint32)
        d_thr = torch.from_numpy(th.view(np.int32)).to(self.device)
        batch = self.perm_batch(T, genes.N, permutations, budget_bytes=1 << 30)
        buf = self._empty((T, batch, self.row_words(genes.N)), torch.int32)
        done = 0
        while done < permutations:
            nb = min(batch, permutations - done)
            self.perm_generate(masks, margins, genes.N, nb, done, seed, out=buf, strata=strata)
            self._check(self.lib.scoary_permute_seq(
                self.h, self._ptr(genes.tiled), self._ptr(buf), self._ptr(crit), self._ptr(d_thr),
                genes.G, T, genes.N, nb, done, self._ptr(r), self._ptr(nstop), self._stream()),
                "scoary_permute_seq")
            done += nb
        return r, nstop

    # -- Westfall-Young minP (spec S7) ------------------------------------------
    def minp_tables(self, counts):
        """The p tables of the traits of ``counts`` (int32 device tensor [T, G, 4], contiguous): every entry is
        k_fisher's own double for the enumerated table.  One 8-byte read-back (the entry count)."""
        torch = _torch()
        counts = counts.contiguous()
        T, G = int(counts.shape[0]), int(counts.shape[1])
        off = self._empty((T * G + 1,), torch.int64)
        lo = self._empty((T, G), torch.int32)
        entries = ctypes.c_int64()
        self._check(self.lib.scoary_minp_plan(self.h, self._ptr(counts), T, G, self._ptr(off), self._ptr(lo),
                                              ctypes.byref(entries), self._stream()), "scoary_minp_plan")
        total = int(entries.value)
        tab = self._empty((total,), torch.float64)
        scratch = self._empty((int(self.lib.scoary_minp_fill_scratch_bytes(total)) // 8,), torch.int64)
        self._check(self.lib.scoary_minp_fill(self.h, self._ptr(counts), self._ptr(off), self._ptr(lo), T, G,
                                              total, self._ptr(scratch), self._ptr(tab), self._stream()),
                    "scoary_minp_fill")
        return MinpTables(off, lo, tab, total)

    def cmh_tables(self, genes, masks, strata, cmh_res):
        """The Westfall-Young tables of the CMH statistic (spec S11; scoary_cmh_minp_plan / _fill): for every (trait,
        gene) u(x) = 1 / (1 + stat(x)) at every pooled count x of its support under the within-stratum shuffles of
        ``strata`` -- MinpTables, the layout permute_minp / permute_stepdown take.  ``masks``: the validity rows
        [T, Wp] of the traits of ``strata``; ``cmh_res``: cmh()'s result for them (its e2 and var are read).  One
        8-byte read-back (the entry count)."""
        e2, var = cmh_res["e2"], cmh_res["var"]
        T, G, _N, off, lo, total, _scratch = self._cmh_support("cmh_tables", genes, masks, strata,
                                                               ((e2, ()), (var, ())), "e2 / var [T, G]")
        tab = self._empty((total,), _torch().float64)
        self._check(self.lib.scoary_cmh_minp_fill(self.h, self._ptr(e2), self._ptr(var), self._ptr(off),
                                                  self._ptr(lo), T, G, total, self._ptr(tab), self._stream()),
                    "scoary_cmh_minp_fill")
        return MinpTables(off, lo, tab, total)

    def _cmh_support(self, who, genes, masks, strata, outputs, what, exact=False):
        """What cmh_tables / cmh_exact / cmh_exact_odds (``who``) start from.  The check: the validity rows ``masks``
        [T, Wp] belong to the traits of ``strata`` and the cmh() outputs they read -- ``outputs``: (tensor, shape after
        [T, G]) pairs, ``what`` names them in the message -- are contiguous and of these T traits x G genes.  Then
        scoary_cmh_minp_plan for these traits: (T, G, N, off int64 [T G + 1], lo int32 [T, G], the entry count, the
        scratch buffer of the segment table).  One 8-byte read-back.  ``exact``: above cmh_exact_max_isolates() the
        plan is left out and the buffers are placeholders."""
        torch = _torch()
        T, G, N = int(masks.shape[0]), genes.G, genes.N
        self._strata_fits(strata, T, N)
        if not masks.is_contiguous() or any(not x.is_contiguous() or tuple(x.shape) != (T, G) + tail
                                            for x, tail in outputs):
            raise ValueError("%s: validity rows [T, Wp] and cmh()'s %s of the same traits, contiguous" % (who, what))
        if exact and N > self.cmh_exact_max_isolates():
            off = self._empty((1,), torch.int64)            # the library refuses the size before it reads anything
            return T, G, N, off, off, T * G, off
        off = self._empty((T * G + 1,), torch.int64)
        lo = self._empty((T, G), torch.int32)
        scratch = self._cmh_scratch(N)
        entries = ctypes.c_int64()
        self._check(self.lib.scoary_cmh_minp_plan(
            self.h, self._ptr(genes.tiled), self._ptr(masks), *self._strata_ptrs(strata), G, T, N, strata.S,
            self._ptr(scratch), self._ptr(off), self._ptr(lo), ctypes.byref(entries), self._stream()),
            "scoary_cmh_minp_plan")
        return T, G, N, off, lo, int(entries.value), scratch

    # -- exact conditional test over the strata (spec S12) ----------------------------
    def cmh_exact_max_isolates(self):
        """The most isolates cmh_exact() takes (the pmf of a gene is held in LDS)."""
        return int(self.lib.scoary_cmh_exact_max_isolates())

    def cmh_exact(self, genes, masks, strata, cmh_res, tables=False):
        """The exact conditional test of every (trait, gene) over the strata of ``strata`` (spec S12;
        scoary_cmh_exact): the pooled count under within-stratum shuffles is the convolution of the strata's
        hypergeometrics.  ``masks``: the validity rows [T, Wp] of the traits of ``strata``; ``cmh_res``: cmh()'s
        result for them (its a and crit are read).  Dict of float64 [T, G] device tensors: p = the two-sided exact
        p of the observed pooled count (probability ordering; Fisher's exact p when there is one stratum), p_region
        = the exact mass of cmh()'s rejection region, the limit of (r_cmh + 1) / (P + 1).  ``tables=True`` adds
        tables = the MinpTables of p over every gene's support (the layout permute_minp / permute_stepdown take);
        p is then read from them.  One 8-byte read-back (the entry count)."""
        torch = _torch()
        a, crit = cmh_res["a"], cmh_res["crit"]
        T, G, N, off, lo, total, scratch = self._cmh_support(
            "cmh_exact", genes, masks, strata, ((a, ()), (crit, (2,))), "a [T, G] / crit [T, G, 2]", exact=True)
        out = {"p": self._empty((T, G), torch.float64), "p_region": self._empty((T, G), torch.float64)}
        tab = self._empty((total,), torch.float64) if tables else None
        self._check(self.lib.scoary_cmh_exact(
            self.h, self._ptr(genes.tiled), self._ptr(masks), *self._strata_ptrs(strata), G, T, N, strata.S,
            self._ptr(a), self._ptr(crit), self._ptr(off), self._ptr(lo), total, self._ptr(out["p"]),
            self._ptr(out["p_region"]), self._ptr(tab) if tables else None, self._ptr(scratch), self._stream()),
            "scoary_cmh_exact")
        if tables:
            out["tables"] = MinpTables(off, lo, tab, total)
        return out

    def cmh_exact_odds(self, genes, masks, strata, cmh_res, level=0.95):
        """The conditional maximum-likelihood estimate of the common odds ratio of every (trait, gene) over the
        strata of ``strata`` and its exact confidence limits at ``level`` (spec S13; scoary_cmh_exact_odds): the
        functionals of cmh_exact()'s pmf that R's mantelhaen.test(exact = TRUE) reports beside its p (fisher.test's
        when there is one stratum).  ``masks`` / ``cmh_res``: as cmh_exact() takes them (a is read).  Dict of float64
        [T, G] device tensors: odds (0 at the lower end of the support, inf at the upper end, nan when the support
        is a single point), lower (0 at the lower end) and upper (inf at the upper end).  One 8-byte read-back."""
        torch = _torch()
        level = float(level)
        if not 0.0 < level < 1.0:
            raise ValueError("cmh_exact_odds: the confidence level must lie inside (0, 1), not %r" % level)
        a = cmh_res["a"]
        T, G, N, off, lo, total, scratch = self._cmh_support(
            "cmh_exact_odds", genes, masks, strata, ((a, ()),), "a [T, G]", exact=True)
        out = {k: self._empty((T, G), torch.float64) for k in ("odds", "lower", "upper")}
        self._check(self.lib.scoary_cmh_exact_odds(
            self.h, self._ptr(genes.tiled), self._ptr(masks), *self._strata_ptrs(strata), G, T, N, strata.S,
            self._ptr(a), self._ptr(off), self._ptr(lo), total, 0.5 * (1.0 - level),
            *(self._ptr(out[k]) for k in ("odds", "lower", "upper")), self._ptr(scratch), self._stream()),
            "scoary_cmh_exact_odds")
        return out

    def _cmh_table_source(self, kind, strata, cmh_res, build):
        """The TableSource ``kind`` over the strata: ``build(t0, t1)`` makes the tables of a trait group; the observed
        values are every gene's own entry at its pooled count cmh_res["a"] (cmh_observed)."""
        def observed(t0, t1, tables):
            return self.cmh_observed(tables, cmh_res["a"][t0:t1])
        return TableSource(kind, strata, build, observed)

    def cmh_exact_source(self, genes, masks, strata, cmh_res):
        """The TableSource of the exact test (spec S12): the tables of cmh_exact() and, as observed values, every
        gene's own entry at its pooled count (cmh_observed), both per trait group -- minp() and minp_stepdown() then
        run over exact stratified p-values.  ``cmh_res``: cmh()'s result for all traits (a and crit are read)."""
        return self._cmh_table_source("cmh_exact", strata, cmh_res, lambda t0, t1: self.cmh_exact(
            genes, masks[t0:t1], strata.rows(t0, t1), {k: cmh_res[k][t0:t1] for k in ("a", "crit")},
            tables=True)["tables"])

    def cmh_observed(self, tables, a):
        """u_obs float64 [T, G] (spec S11 step 4): every gene's own table entry at its pooled count ``a`` (cmh()'s
        int32 [T, G]) -- gathered, never recomputed, so an observed and a permuted gene at the same count tie."""
        torch = _torch()
        T, G = int(a.shape[0]), int(a.shape[1])
        if tuple(tables.lo.shape) != (T, G) or int(tables.off.shape[0]) != T * G + 1:
            raise ValueError("cmh_observed: the tables are those of other traits or genes")
        off = tables.off[:T * G].view(T, G)
        at = (a - tables.lo).to(torch.int64)
        if bool(((at < 0) | (at >= tables.off[1:].view(T, G) - off)).any()):       # one read-back per trait group
            raise ValueError("cmh_observed: a pooled count lies outside its gene's support -- the tables and the "
                             "CMH result do not belong to the same traits and strata")
        return tables.tab[off + at]

    def cmh_source(self, genes, masks, strata, cmh_res):
        """The TableSource of spec S11: the CMH tables of ``strata`` (cmh_tables) and u_obs (cmh_observed), both per
        trait group.  ``cmh_res``: cmh()'s result for all traits (e2, var and a are read)."""
        return self._cmh_table_source("cmh", strata, cmh_res, lambda t0, t1: self.cmh_tables(
            genes, masks[t0:t1], strata.rows(t0, t1), {k: cmh_res[k][t0:t1] for k in ("e2", "var")}))

    def permute_minp(self, genes, perms, tables, minp, P=None, perm_base=0):
        """minp[t, perm_base + i] = min(itself, min over the genes of p_tg(popcount(gene & perms[t, i]))) for the
        label rows ``perms`` (int32 [T, P, Wp], perm_generate's layout).  ``minp``: float64 [T, >= perm_base + P],
        rows contiguous, initialised to 1.0 by the caller."""
        T = int(perms.shape[0])
        if P is None:
            P = int(perms.shape[1])
        if minp.stride(1) != 1 or (T > 1 and minp.stride(0) != minp.shape[1]) or not perms.is_contiguous():
            raise ValueError("permute_minp: minp rows and the label rows must be contiguous")
        self._check(self.lib.scoary_permute_minp(
            self.h, self._ptr(genes.tiled), self._ptr(perms), self._ptr(tables.off), self._ptr(tables.lo),
            self._ptr(tables.tab), genes.G, T, genes.N, int(P), int(perm_base), int(minp.shape[1]),
            self._ptr(minp), self._stream()), "scoary_permute_minp")
        return minp

    def minp_trait_groups(self, counts, table_budget_bytes):
        """Consecutive traits whose p tables together stay under ``table_budget_bytes`` (a trait that is larger on
        its own is a group of one): list of (first, end).  Reads T entry counts back."""
        torch = _torch()
        c = counts.to(torch.int64)
        npos, gm, nval = c[..., 0] + c[..., 1], c[..., 0] + c[..., 2], c.sum(dim=-1)
        size = torch.minimum(npos, gm) - torch.clamp(npos + gm - nval, min=0) + 1
        per_trait = (size.sum(dim=1) * 8).cpu().tolist()
        groups, first, used = [], 0, 0
        for t, b in enumerate(per_trait):
            if t > first and used + b > table_budget_bytes:
                groups.append((first, t))
                first, used = t, 0
            used += b
        groups.append((first, len(per_trait)))
        return groups

    def minp(self, genes, traits, masks, permutations, seed=0, res=None, out=None, perm_range=None,
             table_budget_bytes=8 << 30, label_budget_bytes=8 << 30, plan=None, strata=None, source=None,
             observed_out=None):
        """Westfall-Young minP (spec S7): float64 device tensor [T, permutations], minp[t, pi] = the smallest raw
        Fisher p over the genes of ``genes`` under the S4 labels of (seed, t, pi).  ``res``: an associate() result of
        the same genes and traits (its counts and margins are used; without one they are counted here).
        ``out``: a [T, permutations] tensor to min into (1.0 where nothing has been accumulated yet) -- gene shards and permutation ranges (``perm_range`` = (first, end)) compose by
        min.  The tables of a trait group stay under ``table_budget_bytes`` and the label rows of a batch under
        ``label_budget_bytes``; the result depends on neither.  ``plan``: the TraitPlan of these traits; with
        one, and when all traits fit one group, the tables stay attached to ``genes`` (genes.minp_cache, as the
        index lists do) and later calls with the same plan reuse them: the tables depend on the gene matrix and
        the traits alone, and building them is most of a step (cfg3: 119 of 150 ms).  ``strata``: a StrataPlan
        of these traits -- the labels are those of spec S9 (the tables do not depend on it).  ``source``: a
        TableSource -- the minima are taken over its tables instead of Fisher's p tables (cmh_source: spec S11);
        ``observed_out``: a float64 [T, G] tensor that takes the source's observed values."""
        torch = _torch()
        counts, margins = self._minp_inputs(genes, traits, masks, res, plan)
        if source is None:
            source = self.fisher_source(counts)
        T, P = int(counts.shape[0]), int(permutations)
        if out is None:
            out = torch.ones((T, P), dtype=torch.float64, device=self.device)
        p0, p1 = (0, P) if perm_range is None else (int(perm_range[0]), int(perm_range[1]))

        def launch(t0, t1, tables, perms, nb, done):
            self.permute_minp(genes, perms, tables, out[t0:t1], P=nb, perm_base=done)
        self._minp_batches(genes, masks, counts, margins, p0, p1, seed, table_budget_bytes, label_budget_bytes, plan,
                           launch, source, strata=strata, begin=self._keep_observed(observed_out))
        return out

    @staticmethod
    def _keep_observed(observed_out):
        """The ``begin`` of _minp_batches that copies a group's observed values into ``observed_out`` (None: none)."""
        if observed_out is None:
            return None
        return lambda t0, t1, observed: observed_out[t0:t1].copy_(observed)

    def fisher_source(self, counts, p=None):
        """The TableSource of S7 / S8: Fisher's p tables of ``counts`` and the association step's own p (``p``;
        without one k_fisher is run over the counts when the observed values are first asked for)."""
        own = {"p": p}

        def observed(t0, t1, _tables):
            if own["p"] is None:
                own["p"] = self.fisher(counts.reshape(-1, 4), want_crit=False)[0].view(counts.shape[0],
                                                                                      counts.shape[1])
            return own["p"][t0:t1]
        return TableSource("fisher", None, lambda t0, t1: self.minp_tables(counts[t0:t1]), observed)

    def _minp_inputs(self, genes, traits, masks, res, plan):
        """(counts, margins) of minp() / minp_stepdown(): an associate() result's, or counted here."""
        if plan is not None and not plan.fits(traits, masks):
            raise ValueError("the trait plan was built from other trait / mask tensors")
        if res is not None:
            return res["counts"], res["margins"]
        return self.counts(genes, traits, masks, plan=plan)

    def _minp_batches(self, genes, masks, counts, margins, p0, p1, seed, table_budget_bytes, label_budget_bytes, plan,
                      launch, source, strata=None, begin=None):
        """The loop minp() and minp_stepdown() share: trait groups under the table budget (their tables built by
        ``source``, or taken from / left in genes.minp_cache when there is a plan), label batches under the label
        budget, and per batch ``launch(t0, t1, tables, perms, nb, done)`` -- the traits [t0, t1) with their tables
        and the label rows ``perms`` [t1 - t0, nb, Wp] of the permutations done .. done + nb - 1.  ``begin(t0, t1,
        observed)``: called once per trait group before its first batch, with the source's observed values of the
        group.  The groups are cut by Fisher's support sizes for every source: the support of the pooled count
        under within-stratum shuffles lies inside Fisher's (S11), so the bound holds.  genes.minp_caches has one
        slot per kind of source, checked against the plan, the budget and the source's key: Fisher's tables are
        never handed to a CMH pass, or the reverse, and a step that runs both keeps both."""
        torch = _torch()
        if p1 <= p0:
            return
        N = genes.N
        Wp = self.row_words(N)
        buf = None
        cached = genes.minp_caches.get(source.kind) if plan is not None else None
        if cached is not None and (cached["plan"] is not plan or cached["budget"] != table_budget_bytes
                                   or cached["key"] is not source.key):
            del genes.minp_caches[source.kind]
            cached = None
        groups = cached["groups"] if cached else self.minp_trait_groups(counts, table_budget_bytes)
        for t0, t1 in groups:
            Tg = t1 - t0
            tables = cached["tables"] if cached else source.build(t0, t1)
            if plan is not None and cached is None and len(groups) == 1:
                genes.minp_caches[source.kind] = {"plan": plan, "budget": table_budget_bytes, "groups": groups,
                                                  "tables": tables, "key": source.key}
            if begin is not None:
                begin(t0, t1, source.observed(t0, t1, tables))
            batch = self.perm_batch(Tg, N, p1 - p0, budget_bytes=label_budget_bytes)
            if buf is None or buf.numel() < Tg * batch * Wp:
                buf = self._empty((Tg * batch * Wp,), torch.int32)
            done = p0
            while done < p1:
                nb = min(batch, p1 - done)
                perms = buf[:Tg * nb * Wp].view(Tg, nb, Wp)
                self.perm_generate(masks[t0:t1], margins[t0:t1], N, nb, done, seed, out=perms, trait_base=t0,
                                   strata=strata.rows(t0, t1) if strata is not None else None)
                launch(t0, t1, tables, perms, nb, done)
                done += nb
            del tables

    @staticmethod
    def r_fwer(minp, p):
        """r_fwer[t, g] = #{pi : minp[t, pi] <= p[t, g]} (int32 [T, G]): a sort of every trait's minima and a
        search for every gene's p.  ``p`` must be the association step's own bits (before fisher_scipy)."""
        torch = _torch()
        srt = torch.sort(minp, dim=1).values.contiguous()
        return torch.searchsorted(srt, p.contiguous(), right=True).to(torch.int32)

    def westfall_young(self, genes, traits, masks, permutations, seed, res, fwer=False, stepdown=False,
                       table_budget_bytes=8 << 30, plan=None, strata=None, reduce=None, cmh_fwer=False,
                       cmh_stepdown=False, label_budget_bytes=8 << 30):
        """The Westfall-Young results of the step ``res`` (an associate() result of these genes and traits), composed
        in this one place: dict with minp float64 [T, P], r_fwer int32 [T, G] (``fwer``) and r_fwer_sd int32 [T, G]
        (``stepdown``).  The step-down pass yields the single-step minima as well, so with ``stepdown``
        k_permute_minp is not launched and r_fwer is counted from that pass's minima.  ``reduce``: [T, P] -> [T, P],
        applied to the minima before r_fwer is counted -- dist.all_reduce_min for gene shards, whose minima compose
        by min (the step-down counts do not: minp_stepdown()).  r_fwer is counted on res["p"] as the step produced
        it, k_fisher's own bits: call this before fisher_scipy() rewrites their last ulp.  ``table_budget_bytes``,
        ``label_budget_bytes``, ``plan`` and ``strata`` as in minp().
        ``cmh_fwer`` / ``cmh_stepdown`` (spec S11; ``res`` is a step with cmh=True and ``strata`` its plan): the same
        two passes over the tables of the CMH statistic -- minu float64 [T, P], r_cmh_fwer and r_cmh_fwer_sd int32
        [T, G], counted on u_obs (every gene's own table entry at its pooled count).  The Fisher results are those
        of the call without them, and the reverse."""
        kw = dict(res=res, table_budget_bytes=table_budget_bytes, label_budget_bytes=label_budget_bytes, plan=plan,
                  strata=strata)
        out = {}
        if fwer or stepdown or not (cmh_fwer or cmh_stepdown):
            if stepdown:
                out["r_fwer_sd"], minp = self.minp_stepdown(genes, traits, masks, permutations, seed, **kw)
            else:
                minp = self.minp(genes, traits, masks, permutations, seed, **kw)
            out["minp"] = minp if reduce is None else reduce(minp)
            if fwer:
                out["r_fwer"] = self.r_fwer(out["minp"], res["p"])
        if cmh_fwer or cmh_stepdown:
            if strata is None or "cmh_e2" not in res:
                raise ValueError("cmh_fwer / cmh_stepdown need the result of a step with cmh=True and its strata")
            source = self.cmh_source(genes, masks, strata, self._cmh_of(res))
            u_obs = self._empty(tuple(res["cmh_a"].shape), _torch().float64)
            if cmh_stepdown:
                out["r_cmh_fwer_sd"], out["minu"] = self.minp_stepdown(genes, traits, masks, permutations, seed,
                                                                       source=source, observed_out=u_obs, **kw)
            else:
                out["minu"] = self.minp(genes, traits, masks, permutations, seed, source=source,
                                        observed_out=u_obs, **kw)
            out["u_obs"] = u_obs
            if cmh_fwer:
                out["r_cmh_fwer"] = self.r_fwer(out["minu"], u_obs)
        return out

    # -- Westfall-Young step-down minP (spec S8) ----------------------------------
    def stepdown_chunks(self, G, T, P):
        """Chunks the rank order of G genes is walked in for T traits and P permutations per call
        (scoary_stepdown_chunks: the launch shape's own value)."""
        return int(self.lib.scoary_stepdown_chunks(self.h, int(G), int(T), int(P)))

    def permute_stepdown(self, genes, perms, tables, order, p_sorted, c, minp=None, P=None, perm_base=0):
        """c[t, k] += #{i : min over j >= k of p_{t,order[t,j]}(popcount(gene & perms[t, i])) <= p_sorted[t, k]}: the raw
        step-down counts BY RANK POSITION (spec S8 steps 2-3) of the label rows ``perms`` (int32 [T, P, Wp]).
        ``order`` int32 [T, G] = the gene at every rank, ``p_sorted`` float64 [T, G] = its p, ``c`` int32 [T, G]
        (uint32 bit pattern), zeroed by the caller before the first batch.  ``minp`` (optional): float64
        [T, >= perm_base + P] initialised to 1.0; column perm_base + i takes the minimum over all genes, as
        permute_minp writes it.  Returns c."""
        torch = _torch()
        T = int(perms.shape[0])
        if P is None:
            P = int(perms.shape[1])
        G = genes.G
        if not (perms.is_contiguous() and order.is_contiguous() and p_sorted.is_contiguous() and c.is_contiguous()):
            raise ValueError("permute_stepdown: label rows, order, p_sorted and c must be contiguous")
        if tuple(order.shape) != (T, G) or tuple(p_sorted.shape) != (T, G) or tuple(c.shape) != (T, G) or \
                order.dtype != torch.int32 or p_sorted.dtype != torch.float64 or c.dtype != torch.int32:
            raise ValueError("permute_stepdown: order int32, p_sorted float64 and c int32 must be [T, G]")
        stride = 0
        if minp is not None:
            if minp.stride(1) != 1 or (T > 1 and minp.stride(0) != minp.shape[1]):
                raise ValueError("permute_stepdown: minp rows must be contiguous")
            stride = int(minp.shape[1])
        need = int(self.lib.scoary_stepdown_scratch_bytes(self.h, G, T, genes.N, int(P)))
        scratch = self._empty(((need + 7) // 8,), torch.int64)
        self._check(self.lib.scoary_permute_stepdown(
            self.h, self._ptr(genes.tiled), self._ptr(perms), self._ptr(tables.off), self._ptr(tables.lo),
            self._ptr(tables.tab), self._ptr(order), self._ptr(p_sorted), G, T, genes.N, int(P), int(perm_base),
            stride, self._ptr(minp) if minp is not None else None, self._ptr(c), self._ptr(scratch),
            self._stream()), "scoary_permute_stepdown")
        return c

    def minp_stepdown(self, genes, traits, masks, permutations, seed=0, res=None, table_budget_bytes=8 << 30,
                      label_budget_bytes=8 << 30, plan=None, strata=None, source=None, observed_out=None):
        """Westfall-Young step-down minP (spec S8): (r_sd int32 [T, G], minp float64 [T, permutations]).  Per
        trait the genes are ranked by (p, gene index) -- one stable device sort of the association step's own p --
        and the gene at rank k is compared, per permuted labelling, with the smallest permuted p over the genes at
        rank k and behind; r_sd[t, g] = the number of labellings where that minimum is <= the gene's own p, tied
        genes taking the count of the first of their group and the counts made monotone along the ranks;
        (r_sd + 1) / (P + 1) is the adjusted p, never above the single-step one.  ``minp`` is minp()'s result, bit
        for bit (the same pass produces it).  ``res``, the budgets and ``plan`` as in minp(): the same trait groups,
        label batches and genes.minp_cache; the result depends on none of them.
        On a GENE SHARD this is the step-down within that shard; shards do NOT compose (the successive minimum at
        a global rank mixes the genes of all shards): run it on the whole matrix.  ``strata`` as in minp().
        ``source``: a TableSource -- its tables and observed values take the place of Fisher's p tables and the
        step's p (cmh_source: spec S11, S8 word for word over u); ``observed_out`` as in minp()."""
        torch = _torch()
        counts, margins = self._minp_inputs(genes, traits, masks, res, plan)
        if source is None:
            source = self.fisher_source(counts, res["p"] if res is not None else None)
        T, G, P = int(counts.shape[0]), genes.G, int(permutations)
        ps = self._empty((T, G), torch.float64)
        order32 = self._empty((T, G), torch.int32)
        c = torch.zeros((T, G), dtype=torch.int32, device=self.device)
        minp = torch.ones((T, P), dtype=torch.float64, device=self.device)

        keep = self._keep_observed(observed_out)

        def begin(t0, t1, observed):                                        # ascending (observed value, gene index)
            ps[t0:t1], order32[t0:t1] = torch.sort(observed.contiguous(), dim=1, stable=True)
            if keep is not None:
                keep(t0, t1, observed)

        def launch(t0, t1, tables, perms, nb, done):
            self.permute_stepdown(genes, perms, tables, order32[t0:t1], ps[t0:t1], c[t0:t1], minp=minp[t0:t1], P=nb,
                                  perm_base=done)
        self._minp_batches(genes, masks, counts, margins, 0, P, seed, table_budget_bytes, label_budget_bytes, plan,
                           launch, source, strata=strata, begin=begin)
        # steps 4 and 5: every tie group takes the count of its first position, then the running maximum
        pos = torch.arange(G, device=self.device).expand(T, G)
        first = torch.ones((T, G), dtype=torch.bool, device=self.device)
        first[:, 1:] = ps[:, 1:] != ps[:, :-1]
        head = torch.cummax(torch.where(first, pos, torch.zeros_like(pos)), dim=1).values
        r_rank = torch.cummax(c.gather(1, head), dim=1).values
        r_sd = torch.empty_like(c)
        r_sd.scatter_(1, order32.to(torch.int64), r_rank)
        return r_sd, minp

    def perm_batch(self, T, N, P, budget_bytes=8 << 30):
        """Permutations per generate/permute round so the label buffer stays
        under budget_bytes."""
        per = T * self.row_words(N) * 4
        return int(max(1, min(P, budget_bytes // max(per, 1))))

    # -- the whole hot path ----------------------------------------------------
    def list_batch(self, T, N, permutations, G=0, budget_bytes=8 << 30, scratch_bytes=4 << 30):
        """Permutations per label-tile batch of the list-driven path (multiple of 512): the
        label tiles stay under budget_bytes and the per-(trait, tile, gene) 16-bit counts of
        scoary_permute_lists under scratch_bytes (one count per 512 / 256 / 128 ... permutations,
        trait and gene: 9.8 GB for a cfg5 shard in one batch)."""
        per = max(int(self.lib.scoary_list_tiles_words(N, 512, T)) * 4, 1)    # tile bytes / 512 perms
        batch = (budget_bytes // per) * 512
        if G > 0:
            tile_perms = 32 * self.list_params(N)[0]
            per_tile = 2 * int(T) * (int(G) + 64)                              # count bytes / tile column
            batch = min(batch, max(1, scratch_bytes // per_tile) * tile_perms // 512 * 512)
        return int(max(512, min(-(-permutations // 512) * 512, batch)))

    def workspace(self, genes, T, permutations=0, use_lists=None, perm_buffer=None):
        """Every device buffer one associate() step needs, allocated once: steps that
        reuse it allocate nothing (a precondition for hipGraph capture, and what
        small launch-bound workloads need anyway)."""
        return Workspace(self, genes, T, permutations, self._lists_default(genes, use_lists), perm_buffer)

    def _lists_default(self, genes, use_lists):
        """``use_lists`` of a step; None = the list-driven kernels whenever the matrix has its lists."""
        return (genes.lists is not None and self.lists_supported(genes.N)) if use_lists is None else use_lists

    # -- launch-bound steps: automatic hipGraph replay -----------------------------
    AUTO_GRAPH_MAX_TESTS = 5e8      # ~0.5 ms of kernels at 1e12 tests/s: below it launches dominate

    def auto_graph_eligible(self, genes, T, permutations):
        """A step this small is bound by its five kernel launches (cfg2: 0.112 ms eager, 0.064 ms
        as one graph launch, profiles/r03_bench_cfg2*.json): associate() then records it into a
        hipGraph on its second call with the same buffers and replays it from the third on.
        The recording call synchronises the device once (capture() warms the step up and records
        on a fresh stream); SCOARY_AUTO_GRAPH=0 switches the whole mechanism off."""
        import os
        if os.environ.get("SCOARY_AUTO_GRAPH", "1") == "0":
            return False
        return float(genes.G) * int(T) * max(int(permutations), 1) <= self.AUTO_GRAPH_MAX_TESTS

    def _auto_graph(self, genes, traits, masks, permutations, seed, use_lists, ws, plan, strata=None):
        """The cached-graph path of associate(): returns the result dict, or None for 'run eagerly'."""
        torch = _torch()
        if getattr(self, "_timing", False) or torch.cuda.is_current_stream_capturing():
            return None
        L = genes.lists
        # Everything a recorded step has baked in: the tensors themselves (compared by identity
        # and kept alive by `refs`, so their memory cannot be recycled under the graph), their
        # versions (in-place edits through torch since the recording) and the scalars.
        refs = (genes.tiled, traits, masks, plan, plan.margins, plan.mask_class, plan.buf) + \
            ((L.idx, L.start, L.ngroups, L.order, L.flipped) if L is not None else ()) + \
            ((L.panels,) if L is not None and L.panels is not None else ()) + \
            ((strata, strata.strata, strata.members, strata.offsets, strata.smargins) if strata is not None else ())
        # (a graph recorded without strata is never replayed for a step with strata, or the reverse: the strata
        # plan and its tensors are among the references, and the flag among the scalars)
        scalars = (genes.G, genes.N, int(traits.shape[0]), int(permutations), int(seed), bool(use_lists),
                   getattr(self, "_mfma_mode", "auto"), bool(self.fuse_bfrag), strata is not None,
                   tuple(getattr(x, "_version", 0) for x in refs))
        st = ws.auto
        same = st is not None and st["scalars"] == scalars and len(st["refs"]) == len(refs) and \
            all(a is b for a, b in zip(st["refs"], refs))
        if not same:
            if st is not None and st["graph"] is not None:
                st["graph"].close()                       # waits for its last launch first
            ws.auto = {"refs": refs, "scalars": scalars, "graph": None, "res": None}
            return None                                   # first call with these buffers: eager
        if st["graph"] is None:                           # second call: record (runs the step as well)
            st["graph"], st["res"] = self.capture(genes, traits, masks, permutations, seed, ws,
                                                  use_lists=use_lists, plan=plan, strata=strata)
            # the capture ran on its own stream: order the caller's stream behind it
            torch.cuda.current_stream(self.device).wait_stream(st["graph"].stream)
            return st["res"]
        st["graph"].launch()
        return st["res"]

    def _label_tiles(self, ws, masks, margins, N, nb, base, seed, strata=None, genes=None):
        """One batch of label tiles into ws.tiles: all of them, or -- with label shards -- this
        rank's share followed by the all-gather of the others'.  Returns True if ws.bfrag holds the batch's B
        fragments as well: the workspace has the buffer, the tiles are generated here (gathered tiles go through
        k_mfma_bfrag), and the matrix-core kernel takes slots of this launch (``genes``: the step's matrix)."""
        sh = ws.label_shards
        if sh is None or sh.world == 1:
            fuse = self.fuse_bfrag and ws.bfrag is not None and genes is not None and \
                N <= int(self.lib.scoary_mfma_max_isolates()) and self.mfma_split(genes, masks.shape[0], nb) > 0
            self.perm_generate_tiles(masks, margins, N, nb, base, seed, out=ws.tiles, strata=strata,
                                     bfrag=ws.bfrag if fuse else None)
            return fuse
        nflat, tile_words = self.tiles_per_batch(N, nb, masks.shape[0])
        _per, first, count = sh.share(nflat)
        self.perm_generate_tiles(masks, margins, N, nb, base, seed, out=ws.tiles,
                                 tile_range=(first, count), strata=strata)
        sh.all_gather(ws.tiles, nflat, tile_words)
        return False

    def associate(self, genes, traits, masks, permutations=0, seed=0, perm_buffer=None,
                  use_lists=None, workspace=None, plan=None, graph=None, records=None, fwer=False,
                  table_budget_bytes=8 << 30, stepdown=False, strata=None, cmh=False, cmh_fwer=False,
                  cmh_stepdown=False, cmh_exact=False, cmh_exact_odds=False, cmh_exact_level=0.95,
                  cmh_homogeneity=False):
        """counts -> Fisher -> (optional) permutation exceedance counts.  Returns a dict of device tensors:
        counts [T, G, 4], margins [T, 2], p / odds [T, G], crit [T, G, 2], r [T, G] (uint32 bits in int32) or None.
        ``workspace``: the result tensors are the workspace's, overwritten by the next step that uses it.
        ``plan``: the TraitPlan of these traits (trait_plan, once per trait set); without one every step rebuilds it.
        ``graph``: with a workspace AND a plan a launch-bound step (auto_graph_eligible) is recorded into a hipGraph
        on its second call and replayed afterwards; False keeps it eager.  A step with ``records``, ``fwer``,
        ``stepdown`` or ``cmh`` is never replayed.
        ``records``: an int32 [T, G, 10] tensor the result is also packed into (pack_records): res["records"].
        ``fwer`` / ``stepdown`` (need permutations): res["minp"] float64 [T, P] and res["r_fwer"] / res["r_fwer_sd"]
        int32 [T, G] (westfall_young()); ``table_budget_bytes`` bounds the p tables of a trait group (minp()).
        ``strata``: a StrataPlan of these traits (strata_plan) -- every permutation shuffles the labels within its
        strata only (spec S9), for r and for the Westfall-Young results alike.
        ``cmh`` (needs ``strata``, not permutations): the Cochran-Mantel-Haenszel test over the strata (cmh(), spec
        S10) as res["cmh_stat"], ["cmh_p"], ["cmh_odds"], ["cmh_crit"]; with permutations also res["r_cmh"] int32
        [T, G] (uint32 bits) = the permutations whose pooled count lies in cmh_crit, counted on the same labels as r;
        cmh_e2, cmh_var and cmh_a are cmh()'s e2, var and a.
        ``cmh_fwer`` / ``cmh_stepdown`` (need ``cmh`` and permutations; spec S11): the Westfall-Young passes over the
        CMH statistic -- res["minu"] float64 [T, P], res["u_obs"] float64 [T, G] and res["r_cmh_fwer"] /
        res["r_cmh_fwer_sd"] int32 [T, G] (westfall_young()).
        ``cmh_exact`` (needs ``cmh``, not permutations; spec S12): the exact conditional test over the strata --
        res["cmh_exact_p"] and res["cmh_exact_region_p"] float64 [T, G] (cmh_exact()'s p and p_region).
        ``cmh_exact_odds`` (needs ``cmh``, not permutations; spec S13): the conditional maximum-likelihood odds ratio
        over the strata and its exact confidence limits at ``cmh_exact_level`` -- res["cmh_exact_odds"],
        res["cmh_exact_odds_lower"] and res["cmh_exact_odds_upper"] float64 [T, G] (cmh_exact_odds()).
        ``cmh_homogeneity`` (needs ``cmh``, not permutations; spec S14): the Breslow-Day test of homogeneity of the odds
        ratios over the strata with Tarone's correction -- res["cmh_homog_p"] and res["cmh_homog_stat"] (Tarone's)
        float64 [T, G] and res["cmh_homog_df"] int32 [T, G] (cmh_homogeneity()).
        Every other result is that of the same call without the option, bit for bit."""
        if (fwer or stepdown) and permutations <= 0:
            raise ValueError("fwer=True / stepdown=True need permutations > 0")
        if (cmh_fwer or cmh_stepdown) and (permutations <= 0 or not cmh):
            raise ValueError("cmh_fwer=True / cmh_stepdown=True need cmh=True and permutations > 0")
        if cmh_exact and not cmh:
            raise ValueError("cmh_exact=True needs cmh=True (and its strata)")
        if cmh_exact_odds and not cmh:
            raise ValueError("cmh_exact_odds=True needs cmh=True (and its strata)")
        if cmh_exact_odds and not 0.0 < float(cmh_exact_level) < 1.0:
            raise ValueError("cmh_exact_level must lie inside (0, 1), not %r" % (cmh_exact_level,))
        if cmh_homogeneity and not cmh:
            raise ValueError("cmh_homogeneity=True needs cmh=True (and its strata)")
        if cmh and strata is None:
            raise ValueError("cmh=True needs strata (a StrataPlan of these traits)")
        if strata is not None and (permutations > 0 or cmh):
            self._strata_fits(strata, traits.shape[0], genes.N)
        elif permutations <= 0:
            strata = None
        res = self._associate(genes, traits, masks, permutations, seed, perm_buffer, use_lists,
                              workspace, plan, graph if records is None and not (fwer or stepdown or cmh) else False,
                              strata=strata, cmh=cmh)
        if fwer or stepdown or cmh_fwer or cmh_stepdown:
            res = {**res, **self.westfall_young(genes, traits, masks, permutations, seed, res, fwer, stepdown,
                                                table_budget_bytes, plan, strata, cmh_fwer=cmh_fwer,
                                                cmh_stepdown=cmh_stepdown)}
        if cmh_exact:
            exact = self.cmh_exact(genes, masks, strata, self._cmh_of(res))
            res = {**res, "cmh_exact_p": exact["p"], "cmh_exact_region_p": exact["p_region"]}
        if cmh_exact_odds:
            odds = self.cmh_exact_odds(genes, masks, strata, self._cmh_of(res), level=cmh_exact_level)
            res = {**res, "cmh_exact_odds": odds["odds"], "cmh_exact_odds_lower": odds["lower"],
                   "cmh_exact_odds_upper": odds["upper"]}
        if cmh_homogeneity:
            homog = self.cmh_homogeneity(genes, traits, masks, strata, self._cmh_of(res))
            res = {**res, "cmh_homog_p": homog["p"], "cmh_homog_stat": homog["stat_tarone"],
                   "cmh_homog_df": homog["df"]}
        if records is not None:
            # the exchange records of the step, packed as its last kernel (inside a captured step:
            # one launch less per replay for a gene-sharded rank)
            res = dict(res)
            res["records"] = self.pack_records(res, out=records)
        return res

    def _associate(self, genes, traits, masks, permutations, seed, perm_buffer, use_lists, workspace,
                   plan, graph, strata=None, cmh=False):
        """The step behind associate() (its docstring)."""
        torch = _torch()
        T = traits.shape[0]
        use_lists = self._lists_default(genes, use_lists)
        if use_lists and permutations > 0 and genes.lists is None:
            raise ValueError("use_lists=True but the gene matrix has no index lists: call "
                             "build_lists(genes) once per data set first")
        ws = workspace
        if ws is None:
            ws = Workspace(self, genes, T, permutations, use_lists, perm_buffer)
        elif not ws.fits(genes, T, permutations, use_lists):
            raise ValueError("workspace was made for another problem shape")
        # launch-bound steps with persistent buffers (workspace + plan): replay a cached hipGraph
        # (graph=None: automatic; False: never -- capture() itself, per-kernel timing)
        if graph is None and workspace is not None and plan is not None and perm_buffer is None \
                and ws.label_shards is None and self.auto_graph_eligible(genes, T, permutations):
            res = self._auto_graph(genes, traits, masks, permutations, seed, use_lists, ws, plan, strata)
            if res is not None:
                return res
        counts, margins = self.counts(genes, traits, masks,
                                      out=(ws.counts, ws.margins, ws.mask_class, ws.plan_buf), plan=plan)
        lists = permutations > 0 and use_lists
        if lists:
            # The first batch of label tiles needs only the trait margins, not the
            # Fisher pass: generate it on a side stream while k_fisher runs.  (With a plan the
            # margins are there before k_counts, and the fork could move in front of it: tried,
            # worth 0.2 % at cfg3 and nothing on the launch-bound shapes, while k_counts then
            # shares the chip with the generator and its own duration -- the path's one HBM
            # stream, reported as roofline_k1 -- can no longer be read off the step.)
            # (Round 5, with the 0.04-0.08 ms generator: the overlap is still worth 0.3 % at cfg3 and
            # 2.5 % on a 25 000-gene shard of cfg4, nothing on cfg4 itself.)
            main = torch.cuda.current_stream(self.device)
            side = self._side_stream()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                ready = self._label_tiles(ws, masks, margins, genes.N, min(ws.batch, permutations), 0, seed, strata,
                                          genes)
            p, odds, crit, lcrit = self.fisher(counts, out=(ws.p, ws.odds, ws.crit),
                                               lists=genes.lists, lcrit=ws.lcrit)
        else:
            p, odds, crit = self.fisher(counts, out=(ws.p, ws.odds, ws.crit))
        extra = self._cmh_results(genes, traits, masks, strata, permutations) if cmh else {}
        # every batch of labels is generated once and counted against each (regions, counter) pair of the step:
        # the Fisher regions always (slot order on the list path), the CMH regions (gene order) with cmh
        counted = [({"crit": None, "lcrit": lcrit} if lists else {"crit": crit}, ws.r)]
        if "r_cmh" in extra:
            counted.append(({"crit": extra["cmh_crit"]}, extra["r_cmh"]))
        done = 0
        if lists:
            main.wait_stream(side)
            while done < permutations:
                nb = min(ws.batch, permutations - done)
                if done > 0:
                    ready = self._label_tiles(ws, masks, margins, genes.N, nb, done, seed, strata, genes)
                for regions, r in counted:
                    self.permute_lists(genes, ws.tiles, margins=margins, P=nb, r=r, scratch=ws.scratch,
                                       accumulate=done > 0, bfrag=ws.bfrag, bfrag_ready=ready, **regions)
                done += nb
        elif permutations > 0:
            ws.r.zero_()
            batch = ws.perms.shape[1]
            while done < permutations:
                nb = min(batch, permutations - done)
                self.perm_generate(masks, margins, genes.N, nb, done, seed, out=ws.perms, strata=strata)
                for regions, r in counted:
                    self.permute(genes, ws.perms[:, :nb] if nb == batch else ws.perms, r=r, P=nb, **regions)
                done += nb
        return {"counts": counts, "margins": margins, "p": p, "odds": odds, "crit": crit, "r": ws.r, **extra}

    def _cmh_results(self, genes, traits, masks, strata, permutations):
        """The entries associate(cmh=True) adds to its result: cmh() under the names of the step and, for a step
        with permutations, the zeroed count r_cmh."""
        torch = _torch()
        c = self.cmh(genes, traits, masks, strata)
        out = {"cmh_" + k: c[k] for k in self.CMH_RESULT}
        if permutations > 0:
            out["r_cmh"] = torch.zeros((traits.shape[0], genes.G), dtype=torch.int32, device=self.device)
        return out

    CMH_RESULT = ("stat", "p", "odds", "crit", "e2", "var", "a")        # cmh()'s keys; a step holds them as cmh_*

    @classmethod
    def _cmh_of(cls, res):
        """cmh()'s result read back out of the step ``res`` (_cmh_results' inverse)."""
        return {k: res["cmh_" + k] for k in cls.CMH_RESULT}

    def capture(self, genes, traits, masks, permutations, seed, workspace, use_lists=None, plan=None,
                records=None, strata=None):
        """Record one associate() step into a hipGraph (scoary_graph_*): returns
        (StepGraph, result dict).  The results live in ``workspace``; ``launch()``
        recomputes them with a single graph launch.  The step is run once eagerly
        first (kernel attributes, side stream and lazy module loads happen outside the
        capture)."""
        torch = _torch()
        # checked before anything is launched: the warm-up step below ends in a device
        # synchronize, which is illegal on a capturing stream
        if torch.cuda.is_current_stream_capturing():
            raise _abi.ScoaryHipError("capture(): the current stream is already capturing")
        if workspace.label_shards is not None and workspace.label_shards.world > 1:
            raise _abi.ScoaryHipError("capture(): label shards are active -- their all-gather is a collective "
                                      "and cannot be recorded into a hipGraph")
        self.associate(genes, traits, masks, permutations=permutations, seed=seed,
                       use_lists=use_lists, workspace=workspace, plan=plan, graph=False, records=records,
                       strata=strata)
        torch.cuda.synchronize(self.device)
        stream = torch.cuda.Stream(device=self.device)      # a fresh stream: never mid-capture
        with torch.cuda.stream(stream):
            self._check(self.lib.scoary_graph_begin(self.h, self._stream()), "scoary_graph_begin")
            failed = True
            try:
                res = self.associate(genes, traits, masks, permutations=permutations, seed=seed,
                                     use_lists=use_lists, workspace=workspace, plan=plan, graph=False,
                                     records=records, strata=strata)
                failed = False
            finally:
                # the capture must be ended either way; a graph that came out of a failed step
                # is destroyed here instead of leaking with the exception
                g = ctypes.c_void_p()
                rc = self.lib.scoary_graph_end(self.h, self._stream(), ctypes.byref(g))
                if (failed or rc != 0) and g.value:
                    self.lib.scoary_graph_destroy(g)
                    g = ctypes.c_void_p()
            self._check(rc, "scoary_graph_end")
        return StepGraph(self, g, stream), res

    def pack_records(self, res, nstop=None, out=None):
        """The exchange records of one associate() result (scoary_pack_records): int32
        device tensor [T, G, 10] = counts, p, odds, r, nstop -- the layout of
        scoary_amd.dist.pack_records, produced by one kernel."""
        torch = _torch()
        T, G = res["p"].shape
        if out is None:
            out = self._empty((T, G, 10), torch.int32)
        r = res.get("r")
        self._check(self.lib.scoary_pack_records(
            self.h, self._ptr(res["counts"]), self._ptr(res["p"]), self._ptr(res["odds"]),
            self._ptr(r) if r is not None else None,
            self._ptr(nstop) if nstop is not None else None, T * G, self._ptr(out),
            self._stream()), "scoary_pack_records")
        return out

    # -- --collapse support -----------------------------------------
    def row_hash(self, genes, masks):
        """(T, G, 2) uint64 numpy: 128-bit hash of every gene row AND each
        trait's validity mask."""
        torch = _torch()
        T = masks.shape[0]
        out = self._empty((T, genes.G, 2), torch.int64)
        self._check(self.lib.scoary_row_hash(self.h, self._ptr(genes.tiled), self._ptr(masks),
                                             genes.G, T, genes.N, self._ptr(out), self._stream()),
                    "scoary_row_hash")
        return out.cpu().numpy().view(np.uint64)

    # -- population-structure stage ----------------------------------
    def upgma_merges(self, rows01):
        """rows01: (R, N) 0/1 numpy (rows = isolates, columns = variable genes) -> the
        reference's UPGMA merge order as an (R-1, 2) int32 numpy array, or None when the
        device loop met the degenerate case it hands back (scoary_upgma).  Hamming counts,
        distances and the merge loop stay on the device; only the merge list comes back."""
        torch = _torch()
        R, N = rows01.shape
        counts = self.hamming(rows01, device=True)
        scratch = self._empty(((int(self.lib.scoary_upgma_scratch_bytes(R)) + 7) // 8,), torch.int64)
        merges = self._empty((max(R - 1, 1), 2), torch.int32)
        status = self._empty((1,), torch.int32)
        self._check(self.lib.scoary_upgma(self.h, self._ptr(counts), R, N, self._ptr(scratch),
                                          self._ptr(merges), self._ptr(status), self._stream()),
                    "scoary_upgma")
        if int(status.cpu()[0]) != 0:
            return None
        return merges.cpu().numpy()[:R - 1]

    def hamming(self, rows01, device=False):
        """rows01: (R, N) 0/1 numpy (rows = isolates, columns = variable genes)
        -> (R, R) int32 pairwise Hamming counts (numpy, or the device tensor)."""
        torch = _torch()
        rows01 = np.ascontiguousarray(rows01, dtype=np.uint8)
        R, N = rows01.shape
        bits = pack_bits_rows(rows01)
        gm = self.tile_rows(bits, N)
        vec = self.vecrows(bits, N)
        out = self._empty((R, R), torch.int32)
        self._check(self.lib.scoary_hamming(self.h, self._ptr(gm.tiled), self._ptr(vec), R, N,
                                            self._ptr(out), self._stream()), "scoary_hamming")
        return out if device else out.cpu().numpy()

    def gather_bits(self, rows, index):
        """rows: int32 device tensor [R, Wsrc] of bit rows; index: int32 device
        tensor [K] -> int32 [R, ceil(K/32)] with bit k = source bit index[k]."""
        torch = _torch()
        rows = rows.contiguous()
        R, Wsrc = rows.shape
        K = int(index.shape[0])
        out = self._empty((R, (K + 31) // 32), torch.int32)
        self._check(self.lib.scoary_gather_bits(self.h, self._ptr(rows), R, Wsrc,
                                                self._ptr(index), K, self._ptr(out),
                                                self._stream()), "scoary_gather_bits")
        return out

    def tree_pairs(self, ops, depth, gene_bits, label_bits, K):
        torch = _torch()
        G, L = gene_bits.shape[0], label_bits.shape[0]
        out = self._empty((G, L, 3), torch.int32)
        self._check(self.lib.scoary_tree_pairs(self.h, self._ptr(ops), int(ops.shape[0]),
                                               int(depth), self._ptr(gene_bits),
                                               self._ptr(label_bits), G, L, int(K),
                                               self._ptr(out), self._stream()),
                    "scoary_tree_pairs")
        return out

    def tree_permute(self, ops, depth, gene_bits, label_bits, K, obs):
        torch = _torch()
        G, L = gene_bits.shape[0], label_bits.shape[0]
        out = self._empty((G, L), torch.uint8)
        self._check(self.lib.scoary_tree_permute(self.h, self._ptr(ops), int(ops.shape[0]),
                                                 int(depth), self._ptr(gene_bits),
                                                 self._ptr(label_bits), G, L, int(K),
                                                 self._ptr(obs.contiguous()), self._ptr(out),
                                                 self._stream()), "scoary_tree_permute")
        return out

    # -- quantitative traits: the rank-sum test (spec S15) ---------------------------
    def ranksum_max_isolates(self):
        return int(self.lib.scoary_ranksum_max_isolates())

    def ranksum_plan(self, values):
        """values: float64 [T, N], NaN = missing.  The host ranking of spec S15 as a RankPlan."""
        torch = _torch()
        rc, valid, n, tiesum, groups = rank_rows(values)
        if rc.shape[1] > self.ranksum_max_isolates():
            raise ValueError("ranksum_plan: %d isolates, the rank-sum kernels take at most %d"
                             % (rc.shape[1], self.ranksum_max_isolates()))
        return RankPlan(torch.from_numpy(rc).to(self.device),
                        self.vecrows(pack_bits_rows(valid.astype(np.uint8)), rc.shape[1]),
                        torch.from_numpy(tiesum).to(self.device), rc, valid, n, tiesum, groups,
                        values_host=np.array(values, dtype=np.float64))

    def _ranksum_fits(self, what, genes, plan):
        if genes is not None and genes.N != plan.N:
            raise ValueError("%s: the plan has %d isolates, the gene matrix %d" % (what, plan.N, genes.N))

    def ranksum(self, genes, plan):
        """The observed rank-sum statistic of every (trait, gene): dict of device tensors d (the centred doubled
        rank sum) and m (isolates with the gene and a value) int32 [T, G], auc and p float64 [T, G]; an untestable
        gene has (d 0, auc 0.5, p 1)."""
        torch = _torch()
        self._ranksum_fits("ranksum", genes, plan)
        T, G = plan.T, genes.G
        out = {"d": self._empty((T, G), torch.int32), "m": self._empty((T, G), torch.int32),
               "auc": self._empty((T, G), torch.float64), "p": self._empty((T, G), torch.float64)}
        self._check(self.lib.scoary_ranksum(
            self.h, self._ptr(genes.tiled), self._ptr(plan.rc), self._ptr(plan.valid), self._ptr(plan.tiesum),
            G, T, plan.N, *(self._ptr(out[k]) for k in ("d", "m", "auc", "p")), self._stream()), "scoary_ranksum")
        return out

    def _ranksum_generate(self, src, plan, perm_base, P, seed, bfrag=None):
        """The rows ``src`` int16 [T, N] of ``plan`` shuffled over its valid isolates (spec S15's law) under the
        permutations perm_base .. perm_base + P - 1: int16 [T, P, N], or written into ``bfrag`` as the matrix-core
        kernel's B operand."""
        name = "scoary_ranksum_perm_generate" if bfrag is None else "scoary_ranksum_perm_generate_bfrag"
        out = self._empty((plan.T, int(P), plan.N), _torch().int16) if bfrag is None else bfrag
        self._check(getattr(self.lib, name)(
            self.h, self._ptr(src), self._ptr(plan.valid), plan.T, plan.N, int(P), int(perm_base), 0,
            ctypes.c_uint64(seed), self._ptr(out), self._stream()), name)
        return out

    def ranksum_values(self, plan, perm_base, P, seed):
        """The permuted centred ranks of the permutations perm_base .. perm_base + P - 1: int16 [T, P, N]."""
        return self._ranksum_generate(plan.rc, plan, perm_base, P, seed)

    def ranksum_batch(self, T, N, permutations, budget_bytes=8 << 30):
        """Permutations per batch of ranksum_permute (a multiple of 64): the B operand stays under budget_bytes."""
        per = max(int(self.lib.scoary_ranksum_bfrag_bytes(N, 64, T)), 1)
        return int(max(64, min(-(-permutations // 64) * 64, budget_bytes // per * 64)))

    def _rank_permute(self, what, genes, plan, d_obs, permutations, budget_bytes, generate, maxt=None):
        """The permutation loop of ranksum_permute and vanelteren_permute: batches of ranksum_batch() permutations,
        ``generate(nb, base, bfrag)`` writes a batch as the matrix-core kernel's B operand and k_permute_ranksum adds
        its counts.  ``maxt`` = (iv float64 [T, G], cc, maxs float64 [T, P] of zeros) picks k_rank_maxt instead (spec
        S17): the same counts, and a batch's maxima into its columns of maxs."""
        torch = _torch()
        self._ranksum_fits(what, genes, plan)
        T, G, N, P = plan.T, genes.G, plan.N, int(permutations)
        if tuple(d_obs.shape) != (T, G) or d_obs.dtype != torch.int32 or not d_obs.is_contiguous():
            raise ValueError("%s: d_obs is the observed d, int32 [T, G], contiguous" % what)
        r = torch.zeros((T, G), dtype=torch.int32, device=self.device)
        batch = self.ranksum_batch(T, N, P, budget_bytes)
        bfrag = self._empty((int(self.lib.scoary_ranksum_bfrag_bytes(N, min(batch, P), T)),), torch.uint8)
        for base in range(0, P, batch):
            nb = min(batch, P - base)
            generate(nb, base, bfrag)
            if maxt is None:
                self._check(self.lib.scoary_permute_ranksum(
                    self.h, self._ptr(genes.tiled), self._ptr(bfrag), self._ptr(d_obs), G, T, N, nb, self._ptr(r),
                    self._stream()), "scoary_permute_ranksum")
            else:
                iv, cc, maxs = maxt
                self._check(self.lib.scoary_permute_rank_wy(
                    self.h, self._ptr(genes.tiled), self._ptr(bfrag), self._ptr(d_obs), self._ptr(iv), cc, G, T, N,
                    nb, self._ptr(r), self._ptr(maxs[:, base:]), P, self._stream()), "scoary_permute_rank_wy")
        return r

    def rank_wy_prepare(self, var, d_obs, cc):
        """(iv, s_obs) float64 [T, G] of spec S17 from a rank test's var (0 where untestable) and observed d."""
        torch = _torch()
        T, G = (int(x) for x in d_obs.shape)
        if tuple(var.shape) != (T, G) or var.dtype != torch.float64 or not var.is_contiguous():
            raise ValueError("rank_wy_prepare: var is float64 [T, G], contiguous")
        iv, sobs = self._empty((T, G), torch.float64), self._empty((T, G), torch.float64)
        self._check(self.lib.scoary_rank_wy_prepare(self.h, self._ptr(var), self._ptr(d_obs), int(cc), G, T,
                                                    self._ptr(iv), self._ptr(sobs), self._stream()),
                    "scoary_rank_wy_prepare")
        return iv, sobs

    @staticmethod
    def r_fwer_max(maxs, s_obs):
        """r_fwer[t, g] = #{pi : maxs[t, pi] >= s_obs[t, g]} (int32 [T, G]), doubles compared exactly: a sort of
        every trait's maxima and a search for every gene's statistic (r_fwer()'s counterpart for a maximum)."""
        torch = _torch()
        srt = torch.sort(maxs, dim=1).values.contiguous()
        below = torch.searchsorted(srt, s_obs.contiguous(), right=False)
        return (maxs.shape[1] - below).to(torch.int32)

    def _rank_westfall_young(self, what, genes, plan, res, var, cc, permutations, budget_bytes, generate):
        """Spec S17 over one rank test: (r, r_fwer, maxs) from one pass over the permutations."""
        torch = _torch()
        self._ranksum_fits(what, genes, plan)
        d_obs = res["d"]
        if tuple(d_obs.shape) != (plan.T, genes.G) or d_obs.dtype != torch.int32 or not d_obs.is_contiguous():
            raise ValueError("%s: res is the observed result of these genes and this plan" % what)
        iv, sobs = self.rank_wy_prepare(var, d_obs, cc)
        maxs = torch.zeros((plan.T, int(permutations)), dtype=torch.float64, device=self.device)
        r = self._rank_permute(what, genes, plan, d_obs, permutations, budget_bytes, generate, maxt=(iv, cc, maxs))
        return r, self.r_fwer_max(maxs, sobs), maxs

    def ranksum_permute(self, genes, plan, d_obs, permutations, seed, budget_bytes=8 << 30):
        """r_q int32 [T, G] = #{pi < permutations : |D_pi| >= |d_obs|} under value shuffles (spec S15), in batches
        of ranksum_batch() permutations: the generator writes a batch as the matrix-core kernel's B operand and
        k_permute_ranksum adds its counts."""
        return self._rank_permute("ranksum_permute", genes, plan, d_obs, permutations, budget_bytes,
                                  self._ranksum_generator(plan, seed))

    def _ranksum_generator(self, plan, seed):
        return lambda nb, base, bfrag: self._ranksum_generate(plan.rc, plan, base, nb, seed, bfrag)

    def ranksum_var(self, plan, m):
        """S15's var float64 [T, G] of the observed m (ranksum()'s), 0 where the gene is untestable."""
        torch = _torch()
        T, G = (int(x) for x in m.shape)
        if T != plan.T or m.dtype != torch.int32 or not m.is_contiguous():
            raise ValueError("ranksum_var: m is the observed m, int32 [T, G], contiguous")
        var = self._empty((T, G), torch.float64)
        self._check(self.lib.scoary_ranksum_var(self.h, self._ptr(m), self._ptr(plan.valid), self._ptr(plan.tiesum),
                                                G, T, plan.N, self._ptr(var), self._stream()), "scoary_ranksum_var")
        return var

    def ranksum_westfall_young(self, genes, plan, res, permutations, seed, budget_bytes=8 << 30):
        """Westfall-Young single-step maxT over the rank-sum statistic (spec S17, cc = 1) of the step ``res`` =
        ranksum(genes, plan): (r_q, r_fwer, maxs) -- r_q int32 [T, G] as ranksum_permute returns it, r_fwer int32
        [T, G] = #{pi : maxs[t, pi] >= s_obs[t, g]}, maxs float64 [T, permutations] -- from one pass of k_rank_maxt
        over ranksum_permute's batches."""
        return self._rank_westfall_young("ranksum_westfall_young", genes, plan, res, self.ranksum_var(plan, res["m"]),
                                         1, permutations, budget_bytes, self._ranksum_generator(plan, seed))

    # -- categorical traits: the gene x K-class chi-square test (spec S20) ---------------
    def categorical_max_classes(self):
        return int(self.lib.scoary_categorical_max_classes())

    def categorical_plan(self, codes):
        """codes: integers [T, N], class 1 .. K (K <= categorical_max_classes()), 0 = missing.  The host side of spec
        S20 as a CategoricalPlan."""
        torch = _torch()
        codes, valid, n, nk, classes, weights, limbs = categorical_host(codes)
        if codes.shape[1] > self.ranksum_max_isolates():
            raise ValueError("categorical_plan: %d isolates, the rank-sum generator takes at most %d"
                             % (codes.shape[1], self.ranksum_max_isolates()))
        return CategoricalPlan(torch.from_numpy(codes).to(self.device),
                               self.vecrows(pack_bits_rows(valid.astype(np.uint8)), codes.shape[1]),
                               torch.from_numpy(nk.astype(np.int32)).to(self.device),
                               torch.from_numpy(limbs.view(np.int64)).to(self.device),
                               codes, valid, n, nk, classes, weights, max(1, int(codes.max(initial=0))))

    def categorical(self, genes, plan):
        """The observed 2 x K table and chi-square statistic of every (trait, gene): dict of device tensors a int32
        [T, G, 8] (carriers by class), m int32 [T, G], x2, p and v (Cramer's V) float64 [T, G]; an untestable gene
        has (x2 0, p 1, v 0)."""
        torch = _torch()
        self._ranksum_fits("categorical", genes, plan)
        T, G = plan.T, genes.G
        out = {"a": self._empty((T, G, 8), torch.int32), "m": self._empty((T, G), torch.int32),
               "x2": self._empty((T, G), torch.float64), "p": self._empty((T, G), torch.float64),
               "v": self._empty((T, G), torch.float64)}
        self._check(self.lib.scoary_categorical(
            self.h, self._ptr(genes.tiled), self._ptr(plan.codes), self._ptr(plan.nk), G, T, plan.N, plan.K,
            *(self._ptr(out[k]) for k in ("a", "m", "x2", "p", "v")), self._stream()), "scoary_categorical")
        return out

    def categorical_rows(self, plan, perm_base, P, seed):
        """The permuted code rows of the permutations perm_base .. perm_base + P - 1: int16 [T, P, N], the codes
        shuffled over the isolates that have one by the rank-sum generator (spec S15's law)."""
        return self._ranksum_generate(plan.codes, plan, perm_base, P, seed)

    def categorical_batch(self, T, N, permutations, budget_bytes=8 << 30):
        """Permutations per batch of categorical_permute (a multiple of 64): the code rows stay under budget_bytes."""
        per = max(2 * 64 * int(T) * int(N), 1)
        return int(max(64, min(-(-permutations // 64) * 64, budget_bytes // per * 64)))

    def permute_categorical(self, genes, plan, a_obs, rows, r, maxt=None):
        """r[t, g] += #{rows[t, p] : S_p >= S_obs}, decided in integers (k_cat_permute); rows int16 [T, P, N].
        ``maxt`` = (inv float64 [T, 8], ivm float64 [T, G], maxs float64 [T, >= P], the batch's columns of an array of
        zeros) picks k_cat_maxt instead (spec S22): the same counts, and the batch's maxima into maxs."""
        torch = _torch()
        T, G, N = plan.T, genes.G, plan.N
        self._check_rows_r("permute_categorical", rows, r, T, G, N)
        if maxt is None:
            self._check(self.lib.scoary_permute_categorical(
                self.h, self._ptr(genes.tiled), self._ptr(rows), self._ptr(a_obs), self._ptr(plan.nk),
                self._ptr(plan.w), G, T, N, int(rows.shape[1]), self._ptr(r), self._stream()),
                "scoary_permute_categorical")
            return r
        inv, ivm, maxs = maxt
        if tuple(inv.shape) != (T, 8) or tuple(ivm.shape) != (T, G) or inv.dtype != torch.float64 \
                or ivm.dtype != torch.float64 or not inv.is_contiguous() or not ivm.is_contiguous():
            raise ValueError("permute_categorical: inv and ivm are categorical_wy_prepare's, float64 [T, 8] and [T, G]")
        self._check(self.lib.scoary_permute_cat_wy(
            self.h, self._ptr(genes.tiled), self._ptr(rows), self._ptr(a_obs), self._ptr(plan.nk), self._ptr(plan.w),
            self._ptr(inv), self._ptr(ivm), G, T, N, int(rows.shape[1]), self._ptr(r), self._ptr(maxs),
            self._maxs_stride("permute_categorical", maxs, T, int(rows.shape[1])), self._stream()),
            "scoary_permute_cat_wy")
        return r

    def _maxs_stride(self, what, maxs, T, P):
        """The row stride of a batch's columns of maxs (float64 [T, >= P], unit stride along the permutations)."""
        torch = _torch()
        if maxs.dim() != 2 or maxs.shape[0] != T or maxs.shape[1] < P or maxs.dtype != torch.float64 \
                or maxs.stride(1) != 1 or (T > 1 and maxs.stride(0) < P):
            raise ValueError("%s: maxs is float64 [T, >= P], the batch's columns of a contiguous array" % what)
        return max(int(maxs.stride(0)), P)

    @staticmethod
    def _check_rows_r(what, rows, r, T, G, N):
        """The code rows and the counter of permute_categorical and permute_gcmh."""
        torch = _torch()
        if rows.dim() != 3 or (rows.shape[0], rows.shape[2]) != (T, N) or rows.dtype != torch.int16 \
                or not rows.is_contiguous():
            raise ValueError("%s: rows are int16 [T, P, N], contiguous" % what)
        if tuple(r.shape) != (T, G) or r.dtype != torch.int32 or not r.is_contiguous():
            raise ValueError("%s: r is int32 [T, G], contiguous" % what)

    def _cat_permute(self, genes, plan, permutations, budget_bytes, rows_of, launch):
        """The permutation loop of categorical_permute and gcmh_permute: batches of categorical_batch() permutations,
        ``rows_of(base, nb)`` writes a batch's code rows and ``launch(rows, r, base)`` adds the batch's counts to r
        int32 [T, G], which is returned."""
        T, N, P = plan.T, plan.N, int(permutations)
        r = _torch().zeros((T, genes.G), dtype=_torch().int32, device=self.device)
        batch = self.categorical_batch(T, N, P, budget_bytes)
        for base in range(0, P, batch):
            launch(rows_of(base, min(batch, P - base)), r, base)
        return r

    def categorical_permute(self, genes, plan, a_obs, permutations, seed, budget_bytes=8 << 30, maxt=None):
        """r int32 [T, G] = #{pi < permutations : X2_pi >= X2_obs} under code shuffles (spec S20), in batches of
        categorical_batch() permutations: the rank-sum generator writes a batch's code rows and k_cat_permute adds
        its counts.  ``maxt`` = (inv, ivm, maxs float64 [T, permutations] of zeros) picks k_cat_maxt (spec S22): a
        batch's maxima go into its columns of maxs."""
        self._ranksum_fits("categorical_permute", genes, plan)
        if tuple(a_obs.shape) != (plan.T, genes.G, 8) or a_obs.dtype != _torch().int32 or not a_obs.is_contiguous():
            raise ValueError("categorical_permute: a_obs is the observed a, int32 [T, G, 8], contiguous")
        return self._cat_permute(
            genes, plan, permutations, budget_bytes, lambda base, nb: self.categorical_rows(plan, base, nb, seed),
            lambda rows, r, base: self.permute_categorical(
                genes, plan, a_obs, rows, r, maxt=None if maxt is None else (maxt[0], maxt[1], maxt[2][:, base:])))

    def categorical_wy_prepare(self, plan, a_obs):
        """(inv float64 [T, 8], ivm, s_obs, thr float64 [T, G]) of spec S22 from the observed a of categorical():
        the reciprocals of the class sizes and of m (n - m) (0 where the gene is untestable), the statistic of the
        observed table by the device function of the hot path, and thr = s_obs (1 - 1e-9)."""
        torch = _torch()
        T = plan.T
        if a_obs.dim() != 3 or a_obs.shape[0] != T or a_obs.shape[2] != 8 or a_obs.dtype != torch.int32 \
                or not a_obs.is_contiguous():
            raise ValueError("categorical_wy_prepare: a_obs is the observed a, int32 [T, G, 8], contiguous")
        G = int(a_obs.shape[1])
        inv = self._empty((T, 8), torch.float64)
        ivm, sobs, thr = (self._empty((T, G), torch.float64) for _ in range(3))
        self._check(self.lib.scoary_cat_wy_prepare(
            self.h, self._ptr(a_obs), self._ptr(plan.nk), G, T, plan.K, self._ptr(inv), self._ptr(ivm),
            self._ptr(sobs), self._ptr(thr), self._stream()), "scoary_cat_wy_prepare")
        return inv, ivm, sobs, thr

    def categorical_westfall_young(self, genes, plan, res, permutations, seed, budget_bytes=8 << 30):
        """Westfall-Young single-step maxT over the chi-square statistic (spec S22) of the step ``res`` =
        categorical(genes, plan): (r, r_fwer, maxs) -- r int32 [T, G] as categorical_permute returns it, r_fwer int32
        [T, G] = #{pi : maxs[t, pi] >= thr[t, g]}, maxs float64 [T, permutations] -- from one pass of k_cat_maxt over
        categorical_permute's batches."""
        torch = _torch()
        inv, ivm, _sobs, thr = self.categorical_wy_prepare(plan, res["a"])
        maxs = torch.zeros((plan.T, int(permutations)), dtype=torch.float64, device=self.device)
        r = self.categorical_permute(genes, plan, res["a"], permutations, seed, budget_bytes, maxt=(inv, ivm, maxs))
        return r, self.r_fwer_max(maxs, thr), maxs

    # -- categorical traits over strata: the generalized CMH test (spec S21) -------------
    def gcmh_plan(self, codes, strata):
        """codes: integers [T, N] as categorical_plan takes them; strata: N integers in [0, S), S = the largest + 1,
        shared by all traits.  The host side of spec S21 as a GcmhPlan."""
        torch = _torch()
        st = np.asarray(strata)
        codes = np.asarray(codes)
        if codes.ndim != 2 or st.ndim != 1 or st.shape[0] != codes.shape[1] or st.shape[0] < 1 \
                or not np.issubdtype(st.dtype, np.integer):
            raise ValueError("gcmh_plan: codes must be [T, N] and strata N integers, one per isolate")
        st = st.astype(np.int64)
        N, S = st.shape[0], int(st.max()) + 1
        if st.min() < 0:
            raise ValueError("gcmh_plan: stratum indices must not be negative")
        if S > self.strata_max()[0]:
            raise ValueError("gcmh_plan: %d strata, the kernels take %d (scoary_perm_max_strata)"
                             % (S, self.strata_max()[0]))
        if N > self.ranksum_max_isolates():
            raise ValueError("gcmh_plan: %d isolates, the rank-sum generator takes at most %d"
                             % (N, self.ranksum_max_isolates()))
        codes, valid, n, nk, classes, nsk, l = gcmh_host(codes, st, S)
        members = np.argsort(st, kind="stable").astype(np.int32)
        dev = [torch.from_numpy(np.ascontiguousarray(x)).to(self.device) for x in
               (codes, l, nk.astype(np.int32), nsk.astype(np.int32), st.astype(np.uint16).view(np.int16), members)]
        dev.insert(2, self.vecrows(pack_bits_rows(valid.astype(np.uint8)), N))
        return GcmhPlan(dev, codes, st, S, n, nk, nsk, classes, max(1, int(codes.max(initial=0))))

    def gcmh(self, genes, plan):
        """The observed 2 x K x S table and generalized CMH statistic of every (trait, gene): dict of device tensors a
        int32 [T, G, 8] (carriers by class), m int32 [T, G], e float64 [T, G, 8] (expected carriers by class), form
        float64 [T, G, 35], q, p, thr float64 [T, G] and df int32 [T, G]; an untestable gene has (df 0, q 0, p 1)."""
        torch = _torch()
        self._ranksum_fits("gcmh", genes, plan)
        T, G = plan.T, genes.G
        out = {"a": self._empty((T, G, 8), torch.int32), "m": self._empty((T, G), torch.int32),
               "e": self._empty((T, G, 8), torch.float64), "form": self._empty((T, G, GCMH_FORM), torch.float64),
               "q": self._empty((T, G), torch.float64), "df": self._empty((T, G), torch.int32),
               "p": self._empty((T, G), torch.float64), "thr": self._empty((T, G), torch.float64)}
        scratch = self._cmh_scratch(plan.N)
        self._check(self.lib.scoary_gcmh(
            self.h, self._ptr(genes.tiled), self._ptr(plan.codes), self._ptr(plan.nk), self._ptr(plan.nsk),
            self._ptr(plan.strata), self._ptr(plan.members), G, T, plan.N, plan.K, plan.S,
            *(self._ptr(out[k]) for k in ("a", "m", "e", "form", "q", "df", "p", "thr")), self._ptr(scratch),
            self._stream()), "scoary_gcmh")
        return out

    def gcmh_rows(self, plan, perm_base, P, seed):
        """The permuted code rows of the permutations perm_base .. perm_base + P - 1: int16 [T, P, N], the codes
        shuffled within the strata over the isolates that have one by the van Elteren generator (spec S16's law)."""
        return self._vanelteren_generate(plan.l, plan, perm_base, P, seed)

    def permute_gcmh(self, genes, plan, res, rows, r, maxt=None):
        """r[t, g] += #{rows[t, p] : Q_p >= thr} (k_gcmh_permute); res = gcmh(genes, plan), rows int16 [T, P, N].
        ``maxt`` = maxs float64 [T, >= P], the batch's columns of an array of zeros, picks k_gcmh_maxt instead (spec
        S22): the same counts, and the batch's maxima of Q into maxs."""
        torch = _torch()
        T, G, N = plan.T, genes.G, plan.N
        form, thr = res["form"], res["thr"]
        if tuple(form.shape) != (T, G, GCMH_FORM) or form.dtype != torch.float64 or not form.is_contiguous() \
                or tuple(thr.shape) != (T, G) or thr.dtype != torch.float64 or not thr.is_contiguous():
            raise ValueError("permute_gcmh: res is the observed result of these genes and this plan")
        self._check_rows_r("permute_gcmh", rows, r, T, G, N)
        if maxt is None:
            self._check(self.lib.scoary_permute_gcmh(
                self.h, self._ptr(genes.tiled), self._ptr(rows), self._ptr(form), self._ptr(thr), self._ptr(plan.nk),
                G, T, N, int(rows.shape[1]), self._ptr(r), self._stream()), "scoary_permute_gcmh")
            return r
        self._check(self.lib.scoary_permute_gcmh_wy(
            self.h, self._ptr(genes.tiled), self._ptr(rows), self._ptr(form), self._ptr(thr), self._ptr(plan.nk),
            G, T, N, int(rows.shape[1]), self._ptr(r), self._ptr(maxt),
            self._maxs_stride("permute_gcmh", maxt, T, int(rows.shape[1])), self._stream()), "scoary_permute_gcmh_wy")
        return r

    def gcmh_permute(self, genes, plan, res, permutations, seed, budget_bytes=8 << 30, maxt=None):
        """r int32 [T, G] = #{pi < permutations : Q_pi >= Q_obs (1 - 1e-6)} under code shuffles within the strata
        (spec S21), in categorical_batch() permutations a batch: the van Elteren generator writes a batch's code rows
        and k_gcmh_permute adds its counts.  ``maxt`` = maxs float64 [T, permutations] of zeros picks k_gcmh_maxt (spec
        S22): a batch's maxima go into its columns of maxs."""
        self._ranksum_fits("gcmh_permute", genes, plan)
        return self._cat_permute(
            genes, plan, permutations, budget_bytes, lambda base, nb: self.gcmh_rows(plan, base, nb, seed),
            lambda rows, r, base: self.permute_gcmh(genes, plan, res, rows, r,
                                                    maxt=None if maxt is None else maxt[:, base:]))

    def gcmh_westfall_young(self, genes, plan, res, permutations, seed, budget_bytes=8 << 30):
        """Westfall-Young single-step maxT over the generalized CMH statistic (spec S22) of the step ``res`` =
        gcmh(genes, plan): (r, r_fwer, maxs) -- r int32 [T, G] as gcmh_permute returns it, r_fwer int32 [T, G] =
        #{pi : maxs[t, pi] >= thr[t, g]} with S21's thr, maxs float64 [T, permutations] -- from one pass of
        k_gcmh_maxt over gcmh_permute's batches."""
        torch = _torch()
        maxs = torch.zeros((plan.T, int(permutations)), dtype=torch.float64, device=self.device)
        r = self.gcmh_permute(genes, plan, res, permutations, seed, budget_bytes, maxt=maxs)
        return r, self.r_fwer_max(maxs, res["thr"]), maxs

    # -- quantitative traits: the Hodges-Lehmann shift and its limits (spec S19) --------
    def ranksum_shift_plan(self, values):
        """values: float64 [T, N], NaN = missing (ranksum_plan's).  The sorted values of spec S19 as a RankShiftPlan;
        ValueError for a value above 1e150 in magnitude."""
        torch = _torch()
        xs, pos = shift_rows(values)
        if xs.shape[1] > self.ranksum_max_isolates():
            raise ValueError("ranksum_shift_plan: %d isolates, the rank-sum kernels take at most %d"
                             % (xs.shape[1], self.ranksum_max_isolates()))
        return RankShiftPlan(torch.from_numpy(xs).to(self.device), torch.from_numpy(pos).to(self.device), xs, pos)

    def ranksum_shift(self, genes, plan, res, level=0.95):
        """The Hodges-Lehmann shift of every (trait, gene) of the step ``res`` = ranksum(genes, plan) and its
        confidence limits at ``level`` (spec S19): dict of device tensors shift, lower, upper float64 [T, G] and ca
        int64 [T, G].  The plan's values are sorted once (ranksum_shift_plan) and kept with the plan; ValueError for
        a value above 1e150 in magnitude.  An untestable gene has (0, -inf, +inf, ca 0), and a gene with ca < 1 has
        the limits -inf and +inf."""
        import statistics
        torch = _torch()
        self._ranksum_fits("ranksum_shift", genes, plan)
        if not 0.0 < float(level) < 1.0:
            raise ValueError("ranksum_shift: the confidence level must be inside (0, 1)")
        if plan.shift_plan is None:
            plan.shift_plan = self.ranksum_shift_plan(plan.values_host)
        shift_plan = plan.shift_plan
        T, G = plan.T, genes.G
        m = res["m"]
        if tuple(m.shape) != (T, G) or m.dtype != torch.int32 or not m.is_contiguous():
            raise ValueError("ranksum_shift: res is the observed result of these genes and this plan")
        var = self.ranksum_var(plan, m)
        zq = statistics.NormalDist().inv_cdf(0.5 + float(level) / 2.0)
        out = {k: self._empty((T, G), torch.float64) for k in ("shift", "lower", "upper")}
        out["ca"] = self._empty((T, G), torch.int64)
        self._check(self.lib.scoary_ranksum_shift(
            self.h, self._ptr(genes.tiled), self._ptr(shift_plan.xs), self._ptr(shift_plan.pos),
            self._ptr(plan.valid), self._ptr(m), self._ptr(var), zq, G, T, plan.N,
            *(self._ptr(out[k]) for k in ("shift", "lower", "upper", "ca")), self._stream()), "scoary_ranksum_shift")
        return out

    # -- quantitative traits over strata: the van Elteren test (spec S16) --------------
    def vanelteren_plan(self, values, strata):
        """values: float64 [T, N], NaN = missing; strata: N integers in [0, S), S = the largest + 1.  The host
        ranking, weights, scores and L of spec S16 as a VanElterenPlan."""
        torch = _torch()
        values = np.asarray(values, dtype=np.float64)
        st = np.asarray(strata)
        if values.ndim != 2 or st.ndim != 1 or st.shape[0] != values.shape[1] or st.shape[0] < 1 \
                or not np.issubdtype(st.dtype, np.integer):
            raise ValueError("vanelteren_plan: values must be [T, N] and strata N integers, one per isolate")
        st = st.astype(np.int64)
        N, S = st.shape[0], int(st.max()) + 1
        if st.min() < 0:
            raise ValueError("vanelteren_plan: stratum indices must not be negative")
        if S > self.strata_max()[0]:
            raise ValueError("vanelteren_plan: %d strata, the kernels take %d (scoary_perm_max_strata)"
                             % (S, self.strata_max()[0]))
        if N > self.ranksum_max_isolates():
            raise ValueError("vanelteren_plan: %d isolates, the rank-sum kernels take at most %d"
                             % (N, self.ranksum_max_isolates()))
        score, l, valid, w, n, tiesum, groups, c = vanelteren_rows(values, st, S)
        wn = np.stack([w, n], axis=2).astype(np.int32)
        members = np.argsort(st, kind="stable").astype(np.int32)
        dev = [torch.from_numpy(np.ascontiguousarray(x)).to(self.device) for x in
               (score, l, wn, c, st.astype(np.uint16).view(np.int16), members)]
        dev.insert(2, self.vecrows(pack_bits_rows(valid.astype(np.uint8)), N))
        return VanElterenPlan(dev, score, valid, st, S, w, n, tiesum, groups, c)

    def vanelteren(self, genes, plan):
        """The observed van Elteren statistic of every (trait, gene): dict of device tensors d (the weighted sum of
        the centred doubled within-stratum ranks) and m (isolates with the gene and a value) int32 [T, G], var, auc
        and p float64 [T, G]; an untestable gene has (d 0, var 0, auc 0.5, p 1)."""
        torch = _torch()
        self._ranksum_fits("vanelteren", genes, plan)
        T, G = plan.T, genes.G
        out = {"d": self._empty((T, G), torch.int32), "m": self._empty((T, G), torch.int32),
               "var": self._empty((T, G), torch.float64), "auc": self._empty((T, G), torch.float64),
               "p": self._empty((T, G), torch.float64)}
        scratch = self._cmh_scratch(plan.N)
        self._check(self.lib.scoary_vanelteren(
            self.h, self._ptr(genes.tiled), self._ptr(plan.score), self._ptr(plan.valid), self._ptr(plan.strata),
            self._ptr(plan.members), self._ptr(plan.wn), self._ptr(plan.c), G, T, plan.N, plan.S,
            *(self._ptr(out[k]) for k in ("d", "m", "var", "auc", "p")), self._ptr(scratch), self._stream()),
            "scoary_vanelteren")
        return out

    def vanelteren_values(self, plan, perm_base, P, seed):
        """The score rows of the permutations perm_base .. perm_base + P - 1, shuffled within strata: int16
        [T, P, N]."""
        return self._vanelteren_generate(plan.l, plan, perm_base, P, seed)

    def _vanelteren_generate(self, src, plan, perm_base, P, seed, bfrag=None):
        """_ranksum_generate with the rows shuffled within the plan's strata (spec S16's law)."""
        name = "scoary_vanelteren_perm_generate" if bfrag is None else "scoary_vanelteren_perm_generate_bfrag"
        out = self._empty((plan.T, int(P), plan.N), _torch().int16) if bfrag is None else bfrag
        self._check(getattr(self.lib, name)(
            self.h, self._ptr(src), self._ptr(plan.valid), self._ptr(plan.strata), plan.T, plan.N, plan.S, int(P),
            int(perm_base), 0, ctypes.c_uint64(seed), self._ptr(out), self._stream()), name)
        return out

    def vanelteren_permute(self, genes, plan, d_obs, permutations, seed, budget_bytes=8 << 30):
        """r int32 [T, G] = #{pi < permutations : |D_pi| >= |d_obs|} under value shuffles within the strata (spec
        S16), in ranksum_permute's batches: the stratified generator writes a batch as the B operand and
        k_permute_ranksum adds its counts."""
        return self._rank_permute("vanelteren_permute", genes, plan, d_obs, permutations, budget_bytes,
                                  self._vanelteren_generator(plan, seed))

    def _vanelteren_generator(self, plan, seed):
        return lambda nb, base, bfrag: self._vanelteren_generate(plan.l, plan, base, nb, seed, bfrag)

    def vanelteren_westfall_young(self, genes, plan, res, permutations, seed, budget_bytes=8 << 30):
        """Westfall-Young single-step maxT over the van Elteren statistic (spec S17, cc = 0) of the step ``res`` =
        vanelteren(genes, plan): (r, r_fwer, maxs) as ranksum_westfall_young returns them, the rows shuffled within
        the strata."""
        return self._rank_westfall_young("vanelteren_westfall_young", genes, plan, res, res["var"], 0, permutations,
                                         budget_bytes, self._vanelteren_generator(plan, seed))

    # -- quantitative traits: step-down maxT over the rank statistics (spec S18) --------
    def rank_stepdown_batch(self, G, T, N, permutations, budget_bytes=8 << 30):
        """Permutations per batch of the step-down passes (a multiple of 64): the B operand and gmax -- 8 bytes per
        (trait, group of 64 ranks, column) -- stay under budget_bytes together."""
        per = max(int(self.lib.scoary_ranksum_bfrag_bytes(N, 64, T)), 1) + 8 * int(T) * (self.padded_genes(G) // 64) * 64
        return int(max(64, min(-(-permutations // 64) * 64, budget_bytes // per * 64)))

    @staticmethod
    def rank_stepdown_order(s_obs):
        """Step 1 of spec S18: (order int32 [T, G], ss float64 [T, G]) -- the genes descending by s_obs, ties by
        ascending gene index: one stable descending device sort."""
        torch = _torch()
        ss, order = torch.sort(s_obs.contiguous(), dim=1, descending=True, stable=True)
        return order.to(torch.int32).contiguous(), ss.contiguous()

    def rank_stepdown_gather(self, genes, order32, s_obs, iv, d_obs, N, batch):
        """The scratch of the step-down passes for batches of up to ``batch`` permutations, with every trait's gene
        rows, s_obs, iv and |d_obs| gathered into rank order (k_rank_sd_gather: once per analysis)."""
        torch = _torch()
        T, G = (int(x) for x in d_obs.shape)
        for x, dt, name in ((order32, torch.int32, "order32"), (s_obs, torch.float64, "s_obs"),
                            (iv, torch.float64, "iv"), (d_obs, torch.int32, "d_obs")):
            if tuple(x.shape) != (T, G) or x.dtype != dt or not x.is_contiguous():
                raise ValueError("rank_stepdown_gather: %s is %s [T, G], contiguous" % (name, dt))
        if genes.G != G or genes.N != int(N):
            raise ValueError("rank_stepdown_gather: the gene matrix is not the one of d_obs")
        need = int(self.lib.scoary_rank_stepdown_scratch_bytes(self.h, G, T, int(N), int(batch)))
        scratch = self._empty((need,), torch.uint8)
        self._check(self.lib.scoary_rank_stepdown_gather(
            self.h, self._ptr(genes.tiled), self._ptr(order32), self._ptr(s_obs), self._ptr(iv), self._ptr(d_obs), G, T,
            int(N), self._ptr(scratch), self._stream()), "scoary_rank_stepdown_gather")
        return scratch

    def permute_rank_stepdown(self, scratch, bfrag, cc, G, T, N, P, perm_base, r_rank, c_rank, maxs):
        """One batch of the three step-down launches: the columns perm_base .. perm_base + P - 1 of ``bfrag`` add to
        r_rank and c_rank (int32 [T, G], by rank position) and write their columns of maxs (float64 [T, stride])."""
        self._check(self.lib.scoary_permute_rank_stepdown(
            self.h, self._ptr(scratch), self._ptr(bfrag), int(cc), int(G), int(T), int(N), int(P), int(perm_base),
            self._ptr(r_rank), self._ptr(c_rank), self._ptr(maxs), int(maxs.shape[1]), self._stream()),
            "scoary_permute_rank_stepdown")

    @staticmethod
    def rank_stepdown_tail(c_rank, ss, order32):
        """Steps 4 and 5 of spec S18, minp_stepdown's tail with the comparison mirrored: every position of a group of
        equal ss takes the count of the group's first position, then the running maximum along the ranks, scattered
        to gene order: r_sd int32 [T, G]."""
        torch = _torch()
        T, G = (int(x) for x in c_rank.shape)
        pos = torch.arange(G, device=c_rank.device).expand(T, G)
        first = torch.ones((T, G), dtype=torch.bool, device=c_rank.device)
        first[:, 1:] = ss[:, 1:] != ss[:, :-1]
        head = torch.cummax(torch.where(first, pos, torch.zeros_like(pos)), dim=1).values
        r_rank = torch.cummax(c_rank.gather(1, head), dim=1).values
        r_sd = torch.empty_like(c_rank)
        r_sd.scatter_(1, order32.to(torch.int64), r_rank)
        return r_sd

    def _rank_stepdown(self, what, genes, plan, res, var, cc, permutations, budget_bytes, generate):
        """Spec S18 over one rank test: (r, r_fwer, r_sd, maxs) from one run -- the sort and the gather, the batch
        loop with the test's generator, then the host tail.  k_rank_maxt is not launched: maxs is u[0]."""
        torch = _torch()
        self._ranksum_fits(what, genes, plan)
        d_obs = res["d"]
        T, G, N, P = plan.T, genes.G, plan.N, int(permutations)
        if tuple(d_obs.shape) != (T, G) or d_obs.dtype != torch.int32 or not d_obs.is_contiguous():
            raise ValueError("%s: res is the observed result of these genes and this plan" % what)
        iv, sobs = self.rank_wy_prepare(var, d_obs, cc)
        order32, ss = self.rank_stepdown_order(sobs)
        batch = self.rank_stepdown_batch(G, T, N, P, budget_bytes)
        scratch = self.rank_stepdown_gather(genes, order32, sobs, iv, d_obs, N, min(batch, P))
        bfrag = self._empty((int(self.lib.scoary_ranksum_bfrag_bytes(N, min(batch, P), T)),), torch.uint8)
        r_rank = torch.zeros((T, G), dtype=torch.int32, device=self.device)
        c_rank = torch.zeros((T, G), dtype=torch.int32, device=self.device)
        maxs = torch.zeros((T, P), dtype=torch.float64, device=self.device)
        for base in range(0, P, batch):
            nb = min(batch, P - base)
            generate(nb, base, bfrag)
            self.permute_rank_stepdown(scratch, bfrag, cc, G, T, N, nb, base, r_rank, c_rank, maxs)
        r = torch.empty_like(r_rank)
        r.scatter_(1, order32.to(torch.int64), r_rank)
        return r, self.r_fwer_max(maxs, sobs), self.rank_stepdown_tail(c_rank, ss, order32), maxs

    def ranksum_stepdown(self, genes, plan, res, permutations, seed, budget_bytes=8 << 30):
        """Westfall-Young step-down maxT over the rank-sum statistic (spec S18, cc = 1) of the step ``res`` =
        ranksum(genes, plan): (r_q, r_fwer, r_sd, maxs) -- r_q, r_fwer and maxs as ranksum_westfall_young returns
        them, bit for bit, and r_sd int32 [T, G] with r_q <= r_sd <= r_fwer; (r_sd + 1) / (permutations + 1) is the
        adjusted p.  The step-down is over all genes of the matrix: gene shards do not compose."""
        return self._rank_stepdown("ranksum_stepdown", genes, plan, res, self.ranksum_var(plan, res["m"]), 1,
                                   permutations, budget_bytes, self._ranksum_generator(plan, seed))

    def vanelteren_stepdown(self, genes, plan, res, permutations, seed, budget_bytes=8 << 30):
        """ranksum_stepdown over the van Elteren statistic (spec S18, cc = 0) of the step ``res`` =
        vanelteren(genes, plan), the rows shuffled within the strata."""
        return self._rank_stepdown("vanelteren_stepdown", genes, plan, res, res["var"], 0, permutations, budget_bytes,
                                   self._vanelteren_generator(plan, seed))

    # -- categorical traits: step-down maxT over the chi-square and the gcmh statistic (spec S23) --
    def cat_stepdown_batch(self, G, T, N, permutations, budget_bytes=8 << 30):
        """Permutations per batch of the categorical step-down passes (a multiple of 64): the code rows and gmax -- 8
        bytes per (trait, run of 64 ranks, column) -- stay under budget_bytes together."""
        per = max(2 * 64 * int(T) * int(N), 1) + 8 * int(T) * (-(-int(G) // 1024) * 16) * 64
        return int(max(64, min(-(-permutations // 64) * 64, budget_bytes // per * 64)))

    def _cat_stepdown_scratch(self, what, genes, order32, thr, T, N, batch, gcmh):
        torch = _torch()
        G = genes.G
        for x, dt, name in ((order32, torch.int32, "order32"), (thr, torch.float64, "thr")):
            if tuple(x.shape) != (T, G) or x.dtype != dt or not x.is_contiguous():
                raise ValueError("%s: %s is %s [T, G], contiguous" % (what, name, dt))
        if genes.N != int(N):
            raise ValueError("%s: the gene matrix is not the one of the plan" % what)
        need = int(self.lib.scoary_cat_stepdown_scratch_bytes(self.h, G, T, int(N), int(batch), int(gcmh)))
        if need < 1:
            raise ValueError("%s: sizes outside what the step-down passes take" % what)
        return self._empty((need,), torch.uint8)

    def cat_stepdown_gather(self, genes, order32, a_obs, ivm, thr, N, batch):
        """The scratch of the chi-square step-down passes for batches of up to ``batch`` permutations, with every
        trait's gene rows, a_obs, ivm and thr gathered into position order (k_cat_sd_gather: once per analysis)."""
        torch = _torch()
        T, G = (int(x) for x in thr.shape)
        if tuple(a_obs.shape) != (T, G, 8) or a_obs.dtype != torch.int32 or not a_obs.is_contiguous() \
                or tuple(ivm.shape) != (T, G) or ivm.dtype != torch.float64 or not ivm.is_contiguous():
            raise ValueError("cat_stepdown_gather: a_obs is int32 [T, G, 8] and ivm float64 [T, G], contiguous")
        scratch = self._cat_stepdown_scratch("cat_stepdown_gather", genes, order32, thr, T, N, batch, 0)
        self._check(self.lib.scoary_cat_stepdown_gather(
            self.h, self._ptr(genes.tiled), self._ptr(order32), self._ptr(a_obs), self._ptr(ivm), self._ptr(thr),
            G, T, int(N), self._ptr(scratch), self._stream()), "scoary_cat_stepdown_gather")
        return scratch

    def gcmh_stepdown_gather(self, genes, order32, form, thr, N, batch):
        """cat_stepdown_gather for the generalized CMH test: form float64 [T, G, 35] and thr are gcmh()'s."""
        torch = _torch()
        T, G = (int(x) for x in thr.shape)
        if tuple(form.shape) != (T, G, GCMH_FORM) or form.dtype != torch.float64 or not form.is_contiguous():
            raise ValueError("gcmh_stepdown_gather: form is float64 [T, G, %d], contiguous" % GCMH_FORM)
        scratch = self._cat_stepdown_scratch("gcmh_stepdown_gather", genes, order32, thr, T, N, batch, 1)
        self._check(self.lib.scoary_gcmh_stepdown_gather(
            self.h, self._ptr(genes.tiled), self._ptr(order32), self._ptr(form), self._ptr(thr), G, T, int(N),
            self._ptr(scratch), self._stream()), "scoary_gcmh_stepdown_gather")
        return scratch

    @staticmethod
    def _check_stepdown_batch(what, rows, r_rank, c_rank, maxs, T, G, N):
        torch = _torch()
        AssociationEngine._check_rows_r(what, rows, r_rank, T, G, N)
        AssociationEngine._check_rows_r(what, rows, c_rank, T, G, N)
        if maxs.dim() != 2 or maxs.shape[0] != T or maxs.dtype != torch.float64 or not maxs.is_contiguous():
            raise ValueError("%s: maxs is the whole float64 [T, permutations] array, contiguous" % what)

    def permute_cat_stepdown(self, scratch, plan, inv, rows, G, perm_base, r_rank, c_rank, maxs):
        """One batch of the three chi-square step-down launches: the code rows ``rows`` int16 [T, P, N], the
        permutations perm_base .. perm_base + P - 1, add to r_rank and c_rank (int32 [T, G], by rank position) and
        write their columns of maxs (float64 [T, stride]).  inv: categorical_wy_prepare's."""
        self._check_stepdown_batch("permute_cat_stepdown", rows, r_rank, c_rank, maxs, plan.T, int(G), plan.N)
        self._check(self.lib.scoary_permute_cat_stepdown(
            self.h, self._ptr(scratch), self._ptr(rows), self._ptr(plan.nk), self._ptr(plan.w), self._ptr(inv), int(G),
            plan.T, plan.N, int(rows.shape[1]), int(perm_base), self._ptr(r_rank), self._ptr(c_rank), self._ptr(maxs),
            int(maxs.shape[1]), self._stream()), "scoary_permute_cat_stepdown")

    def permute_gcmh_stepdown(self, scratch, plan, rows, G, perm_base, r_rank, c_rank, maxs):
        """permute_cat_stepdown for the generalized CMH test, the rows shuffled within the strata."""
        self._check_stepdown_batch("permute_gcmh_stepdown", rows, r_rank, c_rank, maxs, plan.T, int(G), plan.N)
        self._check(self.lib.scoary_permute_gcmh_stepdown(
            self.h, self._ptr(scratch), self._ptr(rows), self._ptr(plan.nk), int(G), plan.T, plan.N,
            int(rows.shape[1]), int(perm_base), self._ptr(r_rank), self._ptr(c_rank), self._ptr(maxs),
            int(maxs.shape[1]), self._stream()), "scoary_permute_gcmh_stepdown")

    def _cat_stepdown(self, genes, plan, thr, permutations, budget_bytes, gather, rows_of, launch):
        """Spec S23 over one categorical test: (r, r_fwer, r_sd, maxs) from one run -- the sort by thr and the gather
        (``gather(order32, batch)`` returns the scratch), the batch loop with the test's row generator
        (``launch(scratch, rows, base, r_rank, c_rank, maxs)``), then the host tail.  k_cat_maxt / k_gcmh_maxt are not
        launched: maxs is u[0]."""
        torch = _torch()
        T, G, N, P = plan.T, genes.G, plan.N, int(permutations)
        order32, tt = self.rank_stepdown_order(thr)
        batch = self.cat_stepdown_batch(G, T, N, P, budget_bytes)
        scratch = gather(order32, min(batch, P))
        r_rank = torch.zeros((T, G), dtype=torch.int32, device=self.device)
        c_rank = torch.zeros((T, G), dtype=torch.int32, device=self.device)
        maxs = torch.zeros((T, P), dtype=torch.float64, device=self.device)
        for base in range(0, P, batch):
            launch(scratch, rows_of(base, min(batch, P - base)), base, r_rank, c_rank, maxs)
        r = torch.empty_like(r_rank)
        r.scatter_(1, order32.to(torch.int64), r_rank)
        return r, self.r_fwer_max(maxs, thr), self.rank_stepdown_tail(c_rank, tt, order32), maxs

    def categorical_stepdown(self, genes, plan, res, permutations, seed, budget_bytes=8 << 30):
        """Westfall-Young step-down maxT over the chi-square statistic (spec S23) of the step ``res`` =
        categorical(genes, plan): (r, r_fwer, r_sd, maxs) -- r, r_fwer and maxs as categorical_westfall_young returns
        them, bit for bit, and r_sd int32 [T, G] with r <= r_sd <= r_fwer; (r_sd + 1) / (permutations + 1) is the
        adjusted p.  The step-down is over all genes of the matrix: gene shards do not compose."""
        self._ranksum_fits("categorical_stepdown", genes, plan)
        a_obs = res["a"]
        inv, ivm, _sobs, thr = self.categorical_wy_prepare(plan, a_obs)
        if a_obs.shape[1] != genes.G:
            raise ValueError("categorical_stepdown: res is the observed result of these genes and this plan")
        return self._cat_stepdown(
            genes, plan, thr, permutations, budget_bytes,
            lambda order32, batch: self.cat_stepdown_gather(genes, order32, a_obs, ivm, thr, plan.N, batch),
            lambda base, nb: self.categorical_rows(plan, base, nb, seed),
            lambda scratch, rows, base, r_rank, c_rank, maxs: self.permute_cat_stepdown(
                scratch, plan, inv, rows, genes.G, base, r_rank, c_rank, maxs))

    def gcmh_stepdown(self, genes, plan, res, permutations, seed, budget_bytes=8 << 30):
        """categorical_stepdown over the generalized CMH statistic (spec S23) of the step ``res`` = gcmh(genes, plan),
        the rows shuffled within the strata: r, r_fwer and maxs are gcmh_westfall_young's, bit for bit."""
        torch = _torch()
        self._ranksum_fits("gcmh_stepdown", genes, plan)
        form, thr = res["form"], res["thr"]
        if tuple(thr.shape) != (plan.T, genes.G) or thr.dtype != torch.float64 or not thr.is_contiguous():
            raise ValueError("gcmh_stepdown: res is the observed result of these genes and this plan")
        return self._cat_stepdown(
            genes, plan, thr, permutations, budget_bytes,
            lambda order32, batch: self.gcmh_stepdown_gather(genes, order32, form, thr, plan.N, batch),
            lambda base, nb: self.gcmh_rows(plan, base, nb, seed),
            lambda scratch, rows, base, r_rank, c_rank, maxs: self.permute_gcmh_stepdown(
                scratch, plan, rows, genes.G, base, r_rank, c_rank, maxs))

    # -- covariate-adjusted score tests (spec S24) --------------------------------------
    def score_max_covariates(self):
        return int(self.lib.scoary_score_max_covariates())

    def score_plan(self, values, covariates, kind="logistic"):
        """values: float64 [T, N], nan = missing (0 / 1 for kind "logistic"); covariates: float64 [c, N], nan =
        missing, 0 <= c <= score_max_covariates() (None: intercept only).  The null models of spec S24 as a
        ScorePlan; a trait whose null model S24 refuses is named in plan.skipped and has no testable gene."""
        return self.score_plan_of(score_host(values, covariates, kind), kind)

    def score_plan_of(self, host, kind):
        """The ScorePlan of a dict as score_host returns it: its rows, validity bits, factors and residual sums of
        squares go to the device as they are."""
        torch = _torch()
        N = host["valid"].shape[1]
        dev = (torch.from_numpy(np.ascontiguousarray(host["rows"], dtype=np.float64)).to(self.device),
               self.vecrows(pack_bits_rows(host["valid"].astype(np.uint8)), N),
               torch.from_numpy(np.ascontiguousarray(host["chol"], dtype=np.float64)).to(self.device),
               torch.from_numpy(np.ascontiguousarray(host["rss"], dtype=np.float64)).to(self.device))
        return ScorePlan(dev, host, kind, host["coef"].shape[1])

    def score(self, genes, plan):
        """The score test of every (trait, gene) against the plan's null models: dict of device tensors m int32
        [T, G] (carriers among the trait's valid isolates), U, Vg, beta, se, p float64 [T, G], b float64 [T, G, q] and
        the statistic as ``stat`` (logistic: the score chi-square at one degree of freedom) or ``t`` (linear:
        Student's t at n - q - 1); an untestable gene has (statistic 0, beta 0, se 0, p 1)."""
        torch = _torch()
        if genes.N != plan.N:
            raise ValueError("score: the plan has %d isolates, the gene matrix %d" % (plan.N, genes.N))
        T, G = plan.T, genes.G
        stat = "t" if plan.kind == "linear" else "stat"
        out = {"m": self._empty((T, G), torch.int32), "b": self._empty((T, G, plan.q), torch.float64)}
        out.update((k, self._empty((T, G), torch.float64)) for k in ("U", "Vg", stat, "beta", "se", "p"))
        self._check(self.lib.scoary_score(
            self.h, self._ptr(genes.tiled), self._ptr(plan.rows), self._ptr(plan.valid), self._ptr(plan.chol),
            self._ptr(plan.rss), G, T, plan.N, plan.q, int(plan.kind == "linear"),
            *(self._ptr(out[k]) for k in ("m", "U", "b", "Vg", stat, "beta", "se", "p")), self._stream()),
            "scoary_score")
        return out

    # -- the saddlepoint-corrected p of the logistic score test (spec S25) ----------------
    def score_spa_max_isolates(self):
        return int(self.lib.scoary_score_spa_max_isolates())

    def score_spa(self, genes, plan, score_out, cutoff=2.0):
        """The saddlepoint p of every (trait, gene) behind ``score_out`` = score(genes, plan) of a logistic plan: dict
        of device tensors p float64 [T, G], z and t float64 [T, G, 2] (side 0: the upper tail at +|U|, side 1: the
        lower at -|U|) and status int32 [T, G]: 0 = the score chi-square is below cutoff^2 and p is Score_p's bits,
        1 = the saddlepoint p, 2 = no saddlepoint p could be formed and p is Score_p's bits."""
        torch = _torch()
        if plan.kind != "logistic":
            raise ValueError("score_spa: the saddlepoint p belongs to the logistic score test, the plan is %s"
                             % plan.kind)
        cutoff = float(cutoff)
        if not (np.isfinite(cutoff) and cutoff >= 0.1):
            raise ValueError("score_spa: the cutoff must be a finite number of at least 0.1, not %r" % cutoff)
        if genes.N != plan.N:
            raise ValueError("score_spa: the plan has %d isolates, the gene matrix %d" % (plan.N, genes.N))
        T, G, q = plan.T, genes.G, plan.q
        shapes = {"U": (T, G), "b": (T, G, q), "Vg": (T, G), "stat": (T, G), "p": (T, G)}
        for k, shape in shapes.items():
            if k not in score_out or tuple(score_out[k].shape) != shape or score_out[k].dtype != torch.float64 \
                    or not score_out[k].is_contiguous():
                raise ValueError("score_spa: score_out[%r] must be the float64 %s tensor of score(genes, plan)"
                                 % (k, list(shape)))
        if plan.N > self.score_spa_max_isolates():
            raise ValueError("score_spa: %d isolates, at most %d are taken" % (plan.N, self.score_spa_max_isolates()))
        if plan.spa_rows is None:
            if plan.spa_rows_host is None or plan.spa_rows_host.shape != (T, q + 1, plan.N):
                raise ValueError("score_spa: the plan carries no fitted values and design (score_host's mu and design)")
            plan.spa_rows = torch.from_numpy(plan.spa_rows_host).to(self.device)
        out = {"p": self._empty((T, G), torch.float64), "z": self._empty((T, G, 2), torch.float64),
               "t": self._empty((T, G, 2), torch.float64), "status": self._empty((T, G), torch.int32)}
        scratch = self._empty((int(self.lib.scoary_score_spa_scratch_bytes(G, T)),), torch.uint8)
        self._check(self.lib.scoary_score_spa(
            self.h, self._ptr(genes.tiled), self._ptr(plan.spa_rows), self._ptr(plan.rows), self._ptr(plan.valid),
            self._ptr(plan.chol), *(self._ptr(score_out[k]) for k in ("U", "b", "Vg", "stat", "p")),
            G, T, plan.N, q, cutoff * cutoff, *(self._ptr(out[k]) for k in ("p", "z", "t", "status")),
            self._ptr(scratch), self._stream()), "scoary_score_spa")
        return out

    # -- timing (bench.py) ------------------------------------------------------
    def set_timing(self, on):
        self._check(self.lib.scoary_set_timing(self.h, 1 if on else 0), "scoary_set_timing")
        self._timing = bool(on)          # per-kernel events: steps run eagerly (no graph replay)

    def kernel_ms(self, name):
        ms = ctypes.c_double()
        self._check(self.lib.scoary_last_kernel_ms(self.h, name.encode(), ctypes.byref(ms)),
                    "scoary_last_kernel_ms")
        return ms.value
