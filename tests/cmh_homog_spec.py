"""Spec S14 in plain Python floats: the Breslow-Day statistic of homogeneity of the odds ratios
over per-stratum 2x2 tables, Tarone's correction and the chi-square upper tail -- the same operations in the same
order as the specification, written from it and independently of the kernel.  Also the same functional at 80 digits
(decimal), which picks the root of the quadratic by the stratum's support and not by the sign rule, and the table of
edge genes the device test runs.  A helper, not a test."""
import math
from decimal import Decimal, getcontext

import numpy as np

UNDEFINED = (math.nan, math.nan, 0, 1.0)

# R's UCBAdmissions (cmh_spec.UCB) under S14: psi is cmh_spec.cmh's odds of the six tables
UCB_ANCHOR = {"psi": 0.9046968282586231, "bd": 18.825513705236006, "tarone": 18.82550125205272, "df": 5,
              "p": 0.00207140139788128}


def informative(m, k, n):
    return n > 0 and 0 < k < n and 0 < m < n


def chi2_sf(x, df):
    """Q(df / 2, x / 2) for 1 <= df <= 1023: the finite sum of the tail, all terms positive (plus erfc for an odd df),
    taken outward from its largest term."""
    if not x > 0.0:
        return 1.0
    if x == math.inf:
        return 0.0
    y = x / 2.0
    h, odd = df >> 1, df & 1
    base = math.erfc(math.sqrt(y)) if odd else 0.0
    if h == 0:
        return min(base, 1.0)
    a0 = 0.5 if odd else 0.0                     # term i: y^(a0 + i) e^-y / Gamma(a0 + i + 1), i = 0 .. h - 1
    top_i = int(min(max(math.floor(y - a0), 0.0), float(h - 1)))
    top = math.exp(((a0 + top_i) * math.log(y) - y) - math.lgamma((a0 + top_i) + 1.0))
    total = term = top
    for i in range(top_i, 0, -1):
        term = (term * (a0 + i)) / y
        total += term
        if term < total * 1e-20:
            break
    term = top
    for i in range(top_i + 1, h):
        term = (term * y) / (a0 + i)
        total += term
        if term < total * 1e-20:
            break
    return min(base + total, 1.0)


def homogeneity(tables, psi, trace=None):
    """``tables``: one (a, m, k, n) per stratum in ascending stratum order (cmh_spec's); ``psi``: the double the CMH
    step reports as common odds ratio.  Returns (stat_bd, stat_tarone, df, p).  ``trace``: a list that receives, per
    informative stratum, (the branch of step 4, x, the stratum's support)."""
    if not (psi > 0.0 and psi < math.inf):
        return UNDEFINED
    A1 = 1.0 - psi
    bd = sd = sv = 0.0
    L = 0
    for a, m, k, n in tables:
        if not informative(m, k, n):
            continue
        B = float(n - k - m) + psi * float(k + m)
        C = psi * (float(k) * float(m))
        D = (float((n - k - m) * (n - k - m)) + (psi * psi) * float((k - m) * (k - m))) \
            + (2.0 * psi) * float(k * (n - k) + m * (n - m))
        root = math.sqrt(D)
        if B >= 0.0:
            x = (2.0 * C) / (B + root)
        else:
            x = (root - B) / (2.0 * A1)
        w = ((1.0 / x + 1.0 / (float(k) - x)) + 1.0 / (float(m) - x)) + 1.0 / (float(n - k - m) + x)
        d = float(a) - x
        bd += (d * d) * w
        sd += d
        sv += 1.0 / w
        L += 1
        if trace is not None:
            trace.append(("B<0" if B < 0.0 else "B>=0", x, (max(0, k + m - n), min(k, m))))
    if L < 2:
        return UNDEFINED
    t = bd - (sd * sd) / sv
    tarone = t if t > 0.0 else 0.0
    return bd, tarone, L - 1, chi2_sf(tarone, L - 1)


def exact(tables, psi):
    """(stat_bd, stat_tarone, df) of the same double ``psi`` as Decimals of 80 digits (Tarone's not clamped); the
    fitted count is the root that lies inside the stratum's support.  None where S14 is undefined."""
    if not (psi > 0.0 and psi < math.inf):
        return None
    getcontext().prec = 80
    psi = Decimal(psi)
    bd = sd = sv = Decimal(0)
    L = 0
    for a, m, k, n in tables:
        if not informative(m, k, n):
            continue
        A, B, C = 1 - psi, (n - k - m) + psi * (k + m), -psi * k * m         # A x^2 + B x + C = 0
        lo, hi = max(0, k + m - n), min(k, m)
        if A == 0:
            roots = [-C / B]
        else:
            s = (B * B - 4 * A * C).sqrt()
            roots = [(-B + s) / (2 * A), (-B - s) / (2 * A)]
        inside = [r for r in roots if lo <= r <= hi]
        assert len(inside) == 1, (tables, psi, roots)
        x = inside[0]
        w = 1 / x + 1 / (k - x) + 1 / (m - x) + 1 / (n - k - m + x)
        d = a - x
        bd += d * d * w
        sd += d
        sv += 1 / w
        L += 1
    if L < 2:
        return None
    return bd, bd - sd * sd / sv, L - 1


# -- the edge genes of the device test ----------------------------------------------------------------------------
# (n, k) per stratum -- cmh_cases.EDGE_NK -- and genes as (a, m) per stratum.  Trait 0 has no missing value; trait 1 is
# trait 0 with strata 7 and 3 masked away (n = 0) and all but the first isolate of stratum 0 masked (n = k = 1), as
# cmh_cases.edge_case has it.  What every gene is there for is asserted in test_cmh_homog_spec.py.
EDGE_NK = ((8, 4), (8, 4), (12, 6), (1, 1), (1, 0), (30, 3), (40, 30), (2, 1), (64, 32), (33, 5))
_Z = (0, 0)
EDGE_GENES = {
    "psi_one": ((3, 4), (1, 4), _Z, _Z, _Z, _Z, _Z, _Z, _Z, _Z),                  # R == Q exactly, L = 2
    "b_negative": (_Z, _Z, _Z, _Z, _Z, _Z, (26, 35), _Z, (8, 32), _Z),            # k + m > n and a small psi
    "psi_above_one": (_Z, _Z, (4, 6), _Z, _Z, (1, 4), _Z, _Z, (24, 32), _Z),
    "psi_zero": ((0, 4), _Z, (0, 6), _Z, _Z, _Z, _Z, _Z, _Z, _Z),
    "psi_inf": ((4, 4), _Z, (6, 6), _Z, _Z, _Z, _Z, _Z, _Z, _Z),
    "one_stratum": (_Z, _Z, _Z, _Z, _Z, _Z, _Z, _Z, (20, 32), _Z),                # L = 1
    "with_n_one": (_Z, (2, 5), _Z, (1, 1), (0, 1), (2, 10), _Z, _Z, _Z, (1, 20)),  # the strata of one isolate carry it
    "masked": ((2, 5), _Z, (4, 6), (1, 1), _Z, _Z, _Z, (1, 1), (20, 32), _Z),     # strata 7, 3 and 0 leave with trait 1
    "none": tuple(_Z for _ in EDGE_NK),                                          # in no isolate: psi = nan
    "all": tuple((k, n) for n, k in EDGE_NK),                                    # in every isolate: psi = nan
}


def edge_case():
    """(genes [G, N], traits [2, N], strata [N], names): EDGE_GENES expanded to isolates -- a stratum's k positives
    first, the gene in the first a of them and in the first m - a of the negatives."""
    names = list(EDGE_GENES)
    trait, strata, cols = [], [], {name: [] for name in names}
    for s, (n, k) in enumerate(EDGE_NK):
        trait += [1] * k + [0] * (n - k)
        strata += [s] * n
        for name in names:
            a, m = EDGE_GENES[name][s]
            assert max(0, k + m - n) <= a <= min(k, m), (name, s)
            cols[name] += [1] * a + [0] * (k - a) + [1] * (m - a) + [0] * (n - k - (m - a))
    genes = np.array([cols[name] for name in names], dtype=np.uint8)
    strata = np.array(strata)
    masked = np.array(trait, dtype=np.uint8)
    masked[(strata == 7) | (strata == 3)] = 2
    masked[np.flatnonzero(strata == 0)[1:]] = 2
    return genes, np.stack([np.array(trait, dtype=np.uint8), masked]), strata, names
