"""Spec S20 in plain Python: the Pearson chi-square test of a gene against a label of up to
eight classes and its label permutations.  A helper, not a test; written from the specification, independently of the
kernels and of the engine's host side.  Codes come from strings, counts are exact, X2 is computed in the operation
order the specification fixes, the tail is cmh_homog_spec.chi2_sf, exceedance is decided with fractions.Fraction -- and
a second time, independently, with the limb weights and the sign rule of the specification.  Permuted rows are
ranksum_spec.perm_row applied to the codes."""
import math
from fractions import Fraction

import ranksum_spec as rs
from cmh_homog_spec import chi2_sf

MAX_CLASSES = 8
MAX_ISOLATES = rs.MAX_ISOLATES


def codes_of(labels):
    """labels: a string per isolate, None = missing -> (classes sorted as Python strings, codes: 1 .. K, 0 = missing)."""
    classes = sorted(set(x for x in labels if x is not None))
    number = {c: k + 1 for k, c in enumerate(classes)}
    return classes, [0 if x is None else number[x] for x in labels]


def sizes(codes, K):
    """n_k for k = 1 .. K."""
    return [sum(1 for c in codes if c == k) for k in range(1, K + 1)]


def table(gene, codes, K):
    """a_k = |gene & class k| for k = 1 .. K, of one 0/1 gene row."""
    return [sum(1 for g, c in zip(gene, codes) if g and c == k) for k in range(1, K + 1)]


def testable(a, nk):
    n, m = sum(nk), sum(a)
    return n >= 2 and 0 < m < n and sum(1 for x in nk if x > 0) >= 2


def statistic(a, nk):
    """(testable, X2, df, p, V) of a gene with the table ``a`` against the class sizes ``nk``."""
    n, m = sum(nk), sum(a)
    df = sum(1 for x in nk if x > 0) - 1
    if not testable(a, nk):
        return False, 0.0, df, 1.0, 0.0
    total = 0.0
    for ak, n_k in zip(a, nk):                       # ascending k
        if n_k > 0:
            c = n * ak - m * n_k                     # exact
            total += float(c * c) / float(n_k)
    x2 = total / (float(m) * float(n - m))
    return True, x2, df, chi2_sf(x2, df), math.sqrt(x2 / float(n))


def x2_exact(a, nk):
    """The Pearson chi-square of the 2 x K table as a rational number."""
    n, m = sum(nk), sum(a)
    return sum(Fraction((n * ak - m * n_k) ** 2, n_k) for ak, n_k in zip(a, nk) if n_k > 0) / (m * (n - m))


def s_exact(a, nk):
    return sum(Fraction(ak * ak, n_k) for ak, n_k in zip(a, nk) if n_k > 0)


def s_fp64(a, nk):
    """S = sum a_k^2 / n_k as a plain fp64 sum in ascending k: what an fp64 comparison would look at."""
    total = 0.0
    for ak, n_k in zip(a, nk):
        if n_k > 0:
            total += float(ak * ak) / float(n_k)
    return total


def exceeds(a_perm, a_obs, nk):
    """S_perm >= S_obs in the rationals."""
    return s_exact(a_perm, nk) >= s_exact(a_obs, nk)


def weights(nk):
    """w_k = L / n_k with L = lcm{n_k > 0}; 0 for an empty class."""
    L = 1
    for x in nk:
        if x > 0:
            L = L * x // math.gcd(L, x)
    return [L // x if x > 0 else 0 for x in nk]


def limbs(w):
    """(low, high) 64-bit limbs of a weight."""
    assert 0 <= w < 1 << 112
    return w & 0xFFFFFFFFFFFFFFFF, w >> 64


def exceeds_limbs(a_perm, a_obs, nk):
    """The same decision by the rule the kernel is specified with: H = sum d_k w_hi,k, Lo = sum d_k w_lo,k, both within
    a signed 128-bit integer, and T = H + (Lo >> 64) (arithmetic shift) >= 0."""
    H = Lo = 0
    for ap, ao, w in zip(a_perm, a_obs, weights(nk)):
        d = ap * ap - ao * ao
        assert abs(d) < 1 << 29
        lo, hi = limbs(w)
        assert hi < 1 << 48
        H += d * hi
        Lo += d * lo
    assert abs(H) < 1 << 127 and abs(Lo) < 1 << 127
    return H + (Lo >> 64) >= 0                       # Python's >> of a negative integer is the arithmetic shift


def perm_row(seed, t, pi, codes):
    """The code row of permutation ``pi`` of trait ``t``: S15's shuffle of the codes over the isolates that have one."""
    return rs.perm_row(seed, t, pi, [1 if c else 0 for c in codes], codes)


def r_count(gene, rows, codes, K):
    """#{rows : S_row >= S_obs} of one 0/1 gene row, in the rationals."""
    nk, a_obs = sizes(codes, K), table(gene, codes, K)
    return sum(1 for row in rows if exceeds(table(gene, row, K), a_obs, nk))


def most_enriched(a, nk):
    """The index of the class with the largest a_k / n_k (non-empty classes, integers, ties to the first)."""
    best = None
    for k, (ak, n_k) in enumerate(zip(a, nk)):
        if n_k > 0 and (best is None or Fraction(ak, n_k) > Fraction(a[best], nk[best])):
            best = k
    return best
