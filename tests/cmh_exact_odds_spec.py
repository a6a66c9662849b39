"""Spec S13: the conditional maximum-likelihood estimate of the common odds ratio and its exact
confidence limits, from the pmf f of the pooled count (S12 steps 1 and 2).  Two independent statements, both from the
specification and neither from the kernel: ``restate`` in floating point (S12.float_pmf, terms in the log domain,
bisection in theta = log psi down to the last ulp -- no Newton step, no derivative) and ``brackets``, the EXACT check
of a value in integers (S12.exact_weights; no root finder at all).  A helper, not a test."""
import math
from fractions import Fraction

import numpy as np

import cmh_exact_spec as S12
import cmh_spec as S10

THETA = 700.0                        # theta is searched in [-THETA, THETA]; a root outside is 0 or +inf
WHICH = ("odds", "lower", "upper")


def half_of(level):
    """The double every statement of S13 uses for the tail mass of a limit."""
    assert 0.0 < level < 1.0
    return 0.5 * (1.0 - level)


# -- the floating-point restatement -----------------------------------------------------------------------------
def _roots(lf, xa, kind, half):
    """psi of several root problems over one log-pmf ``lf`` at once (rows: observed index xa[r], kind[r] = 0 the
    estimate, 1 the lower limit, 2 the upper limit).  With x = j - xa and w = exp(lf + theta x - the largest exponent)
    each problem is the sign change of sum c w, increasing in theta:
        c = x (E[X] - A),    c = [x >= 0] - half (P(X >= A) - half),    c = half - [x <= 0] (half - P(X <= A)).
    Bisection in theta over [-THETA, THETA] until the bracket is two neighbouring doubles (or 1e-16 relative); only
    the sign of the sum is used.  One sign over the whole range: 0 or +inf."""
    xa, kind = np.asarray(xa, dtype=np.int64), np.asarray(kind)
    x = np.arange(len(lf), dtype=np.float64)[None, :] - xa[:, None]
    c = np.where(kind[:, None] == 0, x, np.where(kind[:, None] == 1, (x >= 0) - half, half - (x <= 0)))

    def sign(theta):
        e = lf[None, :] + theta[:, None] * x
        w = np.exp(e - e.max(axis=1, keepdims=True))        # lf = -inf (f underflowed): the term is 0
        return np.sign((c * w).sum(axis=1))

    n = len(xa)
    lo, hi = np.full(n, -THETA), np.full(n, THETA)
    psi = np.full(n, np.nan)
    psi[sign(lo) >= 0] = 0.0
    psi[sign(hi) <= 0] = np.inf
    live = np.isnan(psi)
    while live.any():
        mid = 0.5 * (lo + hi)
        s = sign(mid)
        hi = np.where(live & (s > 0), mid, hi)
        lo = np.where(live & (s < 0), mid, lo)
        lo, hi = np.where(live & (s == 0), mid, lo), np.where(live & (s == 0), mid, hi)
        mid = 0.5 * (lo + hi)
        ended = live & (~((lo < mid) & (mid < hi)) | (hi - lo <= 1e-16 * np.maximum(1.0, np.abs(mid))))
        psi[ended] = np.exp(mid[ended])
        live &= ~ended
    return psi


def restate_counts(f, half):
    """(odds, lower, upper) float64 [3, L] of the pmf f (float64 array) at every observed index of its support."""
    L = len(f)
    if L == 1:
        return np.array([[np.nan], [0.0], [np.inf]])
    with np.errstate(divide="ignore"):
        lf = np.log(f)
    out = np.empty((3, L))
    out[0, 0] = out[1, 0] = 0.0                             # A = lo
    out[0, L - 1] = out[2, L - 1] = np.inf                  # A = hi
    todo = [(k, i) for k in range(3) for i in range(L) if not ((i == 0 and k < 2) or (i == L - 1 and k != 1))]
    psi = _roots(lf, [i for _k, i in todo], [k for k, _i in todo], half)
    for (k, i), v in zip(todo, psi):
        out[k, i] = v
    return out


def restate_pmf(f, xa, half):
    """(odds, lower, upper) from the pmf f (float64 array) and the observed index xa."""
    L = len(f)
    if L == 1:
        return math.nan, 0.0, math.inf
    with np.errstate(divide="ignore"):
        lf = np.log(f)
    kinds = [k for k in range(3) if not ((xa == 0 and k < 2) or (xa == L - 1 and k != 1))]
    psi = dict(zip(kinds, _roots(lf, [xa] * len(kinds), kinds, half)))
    return (float(psi.get(0, 0.0 if xa == 0 else math.inf)), float(psi.get(1, 0.0)), float(psi.get(2, math.inf)))


def restate(tables, half):
    """(odds, lower, upper) of one (trait, gene) in floating point: per-stratum (a, m, k, n) as cmh_spec takes them."""
    lo, f = S12.float_pmf(tables)
    return restate_pmf(f, S10.cmh(tables)["a"] - lo, half)


# -- the exact check --------------------------------------------------------------------------------------------
def special(tables, which):
    """The value S13 fixes exactly for ``which`` at these tables, or None where it is a root."""
    shapes = S12.strata_shapes(tables)
    lo, hi = sum(s[3] for s in shapes), sum(s[4] for s in shapes)
    xa, L = sum(a for a, _m, _k, n in tables if n > 0) - lo, hi - lo + 1
    if L == 1:
        return {"odds": math.nan, "lower": 0.0, "upper": math.inf}[which]
    if xa == 0 and which in ("odds", "lower"):
        return 0.0
    if xa == L - 1 and which in ("odds", "upper"):
        return math.inf
    return None


def _value_at(W, xa, half, which, psi):
    """The sign-carrying integer of the monotone function of ``which`` at psi = P / Q (a Fraction): sum over j of
    c_j W_j P^j Q^(L-1-j) with c_j = j - xa for the estimate, and b [j in the tail] - a for a limit (half = a / b)."""
    P, Q, L = psi.numerator, psi.denominator, len(W)
    pw, qw = [1], [1]
    for _ in range(L - 1):
        pw.append(pw[-1] * P)
        qw.append(qw[-1] * Q)
    terms = [W[j] * pw[j] * qw[L - 1 - j] for j in range(L)]
    if which == "odds":
        return sum((j - xa) * terms[j] for j in range(L))
    h = Fraction(half)
    tail = sum(terms[xa:]) if which == "lower" else sum(terms[:xa + 1])
    return h.denominator * tail - h.numerator * sum(terms)


def brackets(tables, half, value, which, eps=1e-12, weights=None):
    """True when the exact root of ``which`` ("odds", "lower", "upper") lies strictly within ``eps`` relative of the
    double ``value`` (finite and positive): the function changes its sign between value (1 - eps) and value (1 + eps),
    evaluated in integers.  Standard library only.  ``weights``: S12.exact_weights(tables), where the caller has it."""
    assert which in WHICH and math.isfinite(value) and value > 0
    lo, W, _D = weights or S12.exact_weights(tables)
    xa = sum(a for a, _m, _k, n in tables if n > 0) - lo
    psi, e = Fraction(value), Fraction(eps)
    below, above = _value_at(W, xa, half, which, psi * (1 - e)), _value_at(W, xa, half, which, psi * (1 + e))
    if which == "upper":                                    # P(X <= A) falls as psi grows
        below, above = -below, -above
    return below < 0 < above


def error_within(tables, half, value, which, eps=1e-12, weights=None):
    """The smallest of eps / 1000, eps / 100, eps / 10 and eps at which ``brackets`` holds, or inf: a figure to print
    (brackets at eps itself is the check)."""
    weights = weights or S12.exact_weights(tables)
    for scale in (1e-3, 1e-2, 1e-1, 1.0):
        if brackets(tables, half, value, which, eps * scale, weights):
            return eps * scale
    return math.inf


def one_sided(tables):
    """(P(X >= A), P(X <= A)) as Fractions from the integer weights."""
    lo, W, D = S12.exact_weights(tables)
    xa = sum(a for a, _m, _k, n in tables if n > 0) - lo
    return Fraction(sum(W[xa:]), D), Fraction(sum(W[:xa + 1]), D)


def check_values(got, want, what=""):
    """Three floats against three floats: special values exactly, the others within 1e-12 relative.  Returns the
    largest relative error."""
    worst = 0.0
    for name, g, w in zip(WHICH, got, want):
        if math.isnan(w):
            assert math.isnan(g), (what, name, g, w)
        elif w == 0.0 or math.isinf(w):
            assert g == w, (what, name, g, w)
        else:
            assert math.isfinite(g) and g > 0, (what, name, g, w)
            rel = abs(g - w) / w
            assert rel <= 1e-12, (what, name, g, w, rel)
            worst = max(worst, rel)
    return worst
