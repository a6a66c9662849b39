"""Spec S12: the exact conditional test over the strata.  Two independent statements of it,
both from the specification and neither from the kernel: the EXACT one in integers / fractions.Fraction (the pmf of
the pooled count as a convolution of hypergeometrics, the p-table under the rule f(y) <= f(x), the mass of S10's
region) and the plain floating-point restatement (ratio recurrence from the mode, every stratum normalised, fp64
convolution, the rule f(y) <= (1 + 1e-7) f(x)).  A helper, not a test."""
from fractions import Fraction
from math import comb

import numpy as np

import cmh_spec as S10

GAMMA = 1.0 + 1e-7
TINY = 1e-290                        # below it the tails may underflow: any value in [0, TINY] stands for the true p


def strata_shapes(tables):
    """(m, k, n, lo_s, hi_s) of the counted strata (n > 0) of per-stratum (a, m, k, n), in their order."""
    return [(m, k, n, max(0, k + m - n), min(k, m)) for _a, m, k, n in tables if n > 0]


# -- exact ------------------------------------------------------------------------------------------------------
def _polymul(A, B):
    """The product of two polynomials with non-negative integer coefficients, exactly: the coefficients packed into
    byte slots wide enough for every coefficient of the product (Kronecker substitution), one integer product."""
    if len(A) * len(B) <= 64:
        out = [0] * (len(A) + len(B) - 1)
        for i, u in enumerate(A):
            for j, v in enumerate(B):
                out[i + j] += u * v
        return out
    width = (max(A).bit_length() + max(B).bit_length() + min(len(A), len(B)).bit_length()) // 8 + 1
    pack = lambda P: int.from_bytes(b"".join(v.to_bytes(width, "little") for v in P), "little")      # noqa: E731
    n = len(A) + len(B) - 1
    raw = (pack(A) * pack(B)).to_bytes(width * (n + 1), "little")
    return [int.from_bytes(raw[i * width:(i + 1) * width], "little") for i in range(n)]


def exact_weights(tables):
    """(lo, W, D): the integer weights W[x - lo] = sum over the splits of x of prod_s C(m_s, x_s) C(n_s - m_s, k_s -
    x_s) for x in [lo, hi], and D = prod_s C(n_s, k_s) = sum W; the pmf is W / D."""
    W, lo, D = [1], 0, 1
    for m, k, n, lo_s, hi_s in strata_shapes(tables):
        w = [comb(m, lo_s) * comb(n - m, k - lo_s)]
        for x in range(lo_s, hi_s):                         # exact: every w is an integer
            w.append(w[-1] * ((m - x) * (k - x)) // ((x + 1) * (n - m - k + x + 1)))
        D *= comb(n, k)
        lo += lo_s
        if len(w) == 1:
            W = [v * w[0] for v in W]
            continue
        W = _polymul(W, w)
    assert sum(W) == D
    return lo, W, D


def exact_p_table(W, D):
    """p(x) = sum{f(y) : f(y) <= f(x)} as Fractions, for every entry of the support."""
    order = sorted(range(len(W)), key=lambda i: W[i])
    upto, run, at = {}, 0, 0
    while at < len(order):                                  # equal weights share their sum
        end = at
        while end < len(order) and W[order[end]] == W[order[at]]:
            run += W[order[end]]
            end += 1
        upto[W[order[at]]] = run
        at = end
    return [Fraction(upto[w], D) for w in W]


def exact_region(lo, W, D, crit):
    """The mass of the counts x with (uint32)(x - base) >= span."""
    return Fraction(sum(w for i, w in enumerate(W) if S10.in_region(crit, lo + i)), D)


def near_tie(W):
    """Two distinct pmf values within 1e-5 relative: the rule with gamma and the exact rule may then part."""
    u = sorted(set(W))
    return any((b - a) * 100000 <= a for a, b in zip(u, u[1:]))


# -- the floating-point restatement -----------------------------------------------------------------------------
def stratum_pmf(m, k, n, lo_s, hi_s):
    """Step 1: the ratio recurrence outward from the mode (weight 1), normalised to sum 1."""
    xm = min(max(((m + 1) * (k + 1)) // (n + 2), lo_s), hi_s)
    f = [0.0] * (hi_s - lo_s + 1)
    f[xm - lo_s] = 1.0
    w = 1.0
    for x in range(xm, hi_s):
        w = (w * (float(m - x) * float(k - x))) / (float(x + 1) * float(n - m - k + x + 1))
        f[x + 1 - lo_s] = w
    w = 1.0
    for x in range(xm, lo_s, -1):
        w = (w * (float(x) * float(n - m - k + x))) / (float(m - x + 1) * float(k - x + 1))
        f[x - 1 - lo_s] = w
    f = np.array(f)
    return f / f.sum()


def float_pmf(tables):
    """Steps 1 and 2: (lo, f float64 array on [lo, hi])."""
    f, lo = np.ones(1), 0
    for m, k, n, lo_s, hi_s in strata_shapes(tables):
        lo += lo_s
        if hi_s > lo_s:
            f = np.convolve(f, stratum_pmf(m, k, n, lo_s, hi_s))
    return lo, f


def float_p_table(f):
    """Step 3: p(x) = min(1, sum{f(y) : f(y) <= gamma f(x)} / sum f); the sums taken from the small end."""
    srt = np.sort(f)
    upto = np.cumsum(srt)
    count = np.searchsorted(srt, GAMMA * f, side="right")
    return np.minimum(1.0, upto[count - 1] / upto[-1])


def float_region(lo, f, crit):
    """Step 4: the mass of the region, 1 for the region (0, 0)."""
    if crit[1] == 0:
        return 1.0
    inside = np.array([bool(S10.in_region(crit, lo + i)) for i in range(len(f))])
    return min(1.0, float(np.sort(f[inside]).sum() / np.sort(f).sum()))


def restate(tables):
    """(lo, p-table float64, p at the observed count, p_region) of one (trait, gene) in floating point."""
    r = S10.cmh(tables)
    lo, f = float_pmf(tables)
    tab = float_p_table(f)
    return lo, tab, tab[r["a"] - lo], float_region(lo, f, r["crit"])


def reference(tables):
    """The same from the exact side, rounded once: (lo, p-table, p at the observed count, p_region, near_tie)."""
    r = S10.cmh(tables)
    lo, W, D = exact_weights(tables)
    tab = np.array([float(p) for p in exact_p_table(W, D)])
    return lo, tab, tab[r["a"] - lo], float(exact_region(lo, W, D, r["crit"])), near_tie(W)


def check(got, want, what=""):
    """The bound of S12: |error| <= 1e-12 everywhere, <= 1e-12 |want| where want >= 1e-290, and 0 <= got <= 1e-290
    below that.  Prints and returns (max absolute, max relative) error."""
    got, want = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64))
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want)
    big = want >= TINY
    rel = np.where(big, err / np.where(big, want, 1.0), 0.0)
    print("cmh exact %s: max abs error %.3e, max relative error %.3e over %d values"
          % (what, err.max(), rel.max(), got.size))
    assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
    assert err.max() <= 1e-12, (what, float(err.max()))
    assert rel.max() <= 1e-12, (what, float(rel.max()))
    assert (got[~big] <= TINY).all()
    return float(err.max()), float(rel.max())


def random_tables(rng, strata, nmax):
    """Random per-stratum (a, m, k, n) with n < nmax (some strata empty), a inside its support."""
    out = []
    for _ in range(strata):
        n = int(rng.integers(0, nmax))
        k, m = int(rng.integers(0, n + 1)), int(rng.integers(0, n + 1))
        a = int(rng.integers(max(0, k + m - n), min(k, m) + 1))
        out.append((a, m, k, n))
    return out
