"""Spec S25 in plain Python: the saddlepoint-corrected p of the logistic score test.  A helper,
not a test; written from the specification, independently of the kernels.  Its inputs are one trait's rows of the plan
(the fitted mu_i and the design columns x_ij, S24's weights, the validity bits, the packed Cholesky factor) and what
S24 returned for one gene (U, b, Vg, stat, p).  Every sum over the isolates is math.fsum of terms from math.expm1 /
log1p, so the restatement's own error is that of the terms; the root is found by Newton steps kept inside a bracket,
run to a step of at most 1e-14 relative or to neighbouring doubles, within 100 evaluations."""
import math

import score_spec as ss

CUTOFF = 2.0                  # the default: SPAtest's
MIN_CUTOFF = 0.1
EDGE = 1e-9                   # |x - s_hi| <= EDGE s_hi: the point mass at the end of the support
STEP = 1e-14
MAX_EVALS = 100
INF = math.inf


def projected(gene, spa_rows, weights, valid, packed, b):
    """[(g~_i, mu_i, w_i)] over the valid isolates in ascending order: L u = b as S24 does, L' c = u, and
    g~_i = g_i - sum_j x_ij c_j as a running subtraction in ascending j (x_i0 = 1).  An isolate without its validity
    bit is left out by that bit, whatever the rows hold there."""
    q = len(b)
    L = ss.unpack(packed, q)
    c = ss.backward(L, ss.forward(L, b))
    out = []
    for i, ok in enumerate(valid):
        if not ok:
            continue
        s = 1.0 if gene[i] else 0.0
        s -= c[0]
        for j in range(1, q):
            s -= spa_rows[1 + j][i] * c[j]
        out.append((s, spa_rows[0][i], weights[i]))
    return out


def cgf(items, t, with_k=True):
    """(K, K', K'') of S = sum g~_i (y_i - mu_i) at t, in the two branches of S25."""
    k0, k1, k2 = [], [], []
    for gt, mu, w in items:
        a = t * gt
        if a <= 0.0:
            e = math.expm1(a)
            d = 1.0 + mu * e
            if with_k:
                k0.append(math.log1p(mu * e) - a * mu)
            k1.append(gt * w * e / d)
        else:
            e = math.expm1(-a)
            d = 1.0 + (1.0 - mu) * e
            if with_k:
                k0.append(math.log1p((1.0 - mu) * e) + a * (1.0 - mu))
            k1.append(gt * w * (-e) / d)
        k2.append(w * gt * gt * (e + 1.0) / (d * d))
    return math.fsum(k0), math.fsum(k1), math.fsum(k2)


def support(items):
    """(s_lo, s_hi): the ends of the support of S."""
    hi = math.fsum(gt * (1.0 - mu) if gt > 0.0 else -gt * mu for gt, mu, _w in items)
    lo = -math.fsum(gt * mu if gt > 0.0 else -gt * (1.0 - mu) for gt, mu, _w in items)
    return lo, hi


def point_mass(items, upper):
    """P(S = s_hi) (upper) or P(S = s_lo): every isolate at the value that pushes S that way."""
    logs = []
    for gt, mu, _w in items:
        if gt != 0.0:
            logs.append(math.log(mu) if (gt > 0.0) == upper else math.log1p(-mu))
    return math.exp(math.fsum(logs))


def root(items, x, Vg):
    """The root of K'(t) = x, x != 0, or None where the search does not end within MAX_EVALS evaluations."""
    lo, hi = (0.0, INF) if x > 0.0 else (-INF, 0.0)
    t = x / Vg                                        # the Newton step from 0: K'(0) = 0, K''(0) = Vg
    for _ in range(MAX_EVALS):
        _k, k1, k2 = cgf(items, t, with_k=False)
        f = k1 - x
        if f > 0.0:
            hi = t
        else:
            lo = t
        tn = t - f / k2 if k2 > 0.0 else math.nan
        if not lo < tn < hi:
            tn = 4.0 * t if math.isinf(lo) or math.isinf(hi) else 0.5 * (lo + hi)
        if abs(tn - t) <= STEP * abs(tn):
            return tn
        if not (math.isinf(lo) or math.isinf(hi)) and math.nextafter(lo, hi) >= hi:
            return tn
        t = tn
    return None


def side(items, x, s_end, upper, Vg):
    """One side of S25 at x = +|U| (upper, s_end = s_hi) or -|U| (s_end = s_lo): (tail, t^, z) or None for the
    fallback."""
    far = INF if upper else -INF
    ax, aend = abs(x), abs(s_end)
    if ax > aend * (1.0 + EDGE):
        return 0.0, far, 0.0
    if abs(ax - aend) <= EDGE * aend:
        return point_mass(items, upper), far, 0.0
    t = root(items, x, Vg)
    if t is None:
        return None
    k0, _k1, k2 = cgf(items, t)
    q2 = t * x - k0
    if not (0.0 < q2 < INF and 0.0 < k2 < INF):
        return None
    omega = math.copysign(math.sqrt(2.0 * q2), t)
    v = t * math.sqrt(k2)
    ratio = v / omega
    if not 0.0 < ratio < INF:
        return None
    z = omega + math.log(ratio) / omega
    if not (z > 0.0) == (x > 0.0) or z == 0.0 or math.isnan(z):
        return None
    return 0.5 * math.erfc(abs(z) / math.sqrt(2.0)), t, z


def spa(gene, spa_rows, weights, valid, packed, U, b, Vg, stat, p, cutoff=CUTOFF):
    """dict(p, z [2], t [2], status) of one (trait, gene): side 0 is x = +|U|, side 1 x = -|U|; at status 1 also
    tails [2], the two summands of p."""
    if not (math.isfinite(cutoff) and cutoff >= MIN_CUTOFF):
        raise ValueError("cutoff")
    if stat < cutoff * cutoff:
        return dict(p=p, z=[0.0, 0.0], t=[0.0, 0.0], status=0)
    items = projected(gene, spa_rows, weights, valid, packed, b)
    s_lo, s_hi = support(items)
    sides = [side(items, abs(U), s_hi, True, Vg), side(items, -abs(U), s_lo, False, Vg)]
    if None in sides:
        return dict(p=p, z=[s[2] if s else 0.0 for s in sides], t=[s[1] if s else 0.0 for s in sides], status=2)
    return dict(p=min(1.0, sides[0][0] + sides[1][0]), z=[s[2] for s in sides], t=[s[1] for s in sides], status=1,
                tails=[s[0] for s in sides])
