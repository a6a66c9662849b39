"""Spec S21 in plain Python: the generalized Cochran-Mantel-Haenszel test of a gene against a
label of up to eight classes over strata (the 2 x K x S table) and its label permutations within the strata.  A helper,
not a test; written from the specification, independently of the kernels and of the engine's host side.  The float
route does the operations of the specification in its order; the rational route (fractions.Fraction) is the reference
it is held to; ``*_many`` are the float route over many genes at once in numpy (the same IEEE operations, element by
element), for the GPU tests.  Permuted rows are vanelteren_spec.perm_row applied to the codes."""
from fractions import Fraction

import numpy as np

import vanelteren_spec as vs
from cmh_homog_spec import chi2_sf

MAX_CLASSES = 8
NC = MAX_CLASSES - 1                # contrasts: every class but the last non-empty one
FORM = NC + NC * (NC - 1) // 2 + NC            # E[7], f[21], invp[7]
THETA = 1e-8                        # the pivot rule's threshold (measured: test_gcmh_spec.py, DESIGN S21)
TAU = 1e-6                          # the exceedance band (S10's)
ONE_MINUS_TAU = 1.0 - TAU


def fidx(i, j):
    """The place of the multiplier f_ij (j < i) in f[21]: rows one after the other."""
    return i * (i - 1) // 2 + j


def margins(codes, strata, S):
    """n_sk [S][8] of one trait: codes 1 .. 8 (0 = missing), strata in [0, S)."""
    nsk = [[0] * MAX_CLASSES for _ in range(S)]
    for c, s in zip(codes, strata):
        if c:
            nsk[s][c - 1] += 1
    return nsk


def klast(nsk):
    """The last class (1-based) with n_k > 0; 0 without any."""
    last = 0
    for row in nsk:
        for k, x in enumerate(row):
            if x > 0:
                last = max(last, k + 1)
    return last


def counts(gene, codes, strata, S):
    """(a [8] pooled, m_s [S]) of one 0/1 gene row."""
    a, ms = [0] * MAX_CLASSES, [0] * S
    for g, c, s in zip(gene, codes, strata):
        if g and c:
            a[c - 1] += 1
            ms[s] += 1
    return a, ms


def moments(ms, nsk):
    """(E [8], V [7][7] lower triangle) in fp64, ascending strata, every operation rounded on its own."""
    E = [0.0] * MAX_CLASSES
    V = [[0.0] * NC for _ in range(NC)]
    for m, row in zip(ms, nsk):
        n = sum(row)
        if n == 0:
            continue
        for k in range(MAX_CLASSES):
            E[k] += float(m * row[k]) / float(n)
        if n >= 2:
            c = (float(m) * float(n - m)) / ((float(n) * float(n)) * float(n - 1))
            for j in range(NC):
                for k in range(j + 1):
                    B = (n * row[j] if j == k else 0) - row[j] * row[k]
                    V[j][k] += c * float(B)
    return E, V


def factor(E, V, nc, theta=THETA, trace=None):
    """The form of a (trait, gene) -- FORM doubles: E[7], f[21], invp[7] -- and df.  LDL' without pivoting in class
    order over the contrasts j < nc; the rows from nc on count as zero.  ``trace``: a list that takes every (pivot,
    diagonal entry)."""
    f, invp, df = [0.0] * (NC * (NC - 1) // 2), [0.0] * NC, 0
    u = [[0.0] * NC for _ in range(NC)]
    for j in range(NC):
        for k in range(j):
            x = V[j][k] if j < nc else 0.0
            for l in range(k):
                x = x - u[j][l] * f[fidx(k, l)]
            u[j][k] = x
            f[fidx(j, k)] = x * invp[k]
        vjj = V[j][j] if j < nc else 0.0
        p = vjj
        for k in range(j):
            p = p - u[j][k] * f[fidx(j, k)]
        if trace is not None:
            trace.append((p, vjj))
        if not p <= theta * vjj:
            invp[j] = 1.0 / p
            df += 1
    return [E[j] if j < nc else 0.0 for j in range(NC)] + f + invp, df


def q_of(a, form):
    """Q of the pooled counts a (the first seven are read) under a form."""
    E, f, invp = form[:NC], form[NC:FORM - NC], form[FORM - NC:]
    y = [0.0] * NC
    for i in range(NC):
        x = float(a[i]) - E[i]
        for j in range(i):
            x = x - f[fidx(i, j)] * y[j]
        y[i] = x
    q = 0.0
    for j in range(NC):
        q += (y[j] * y[j]) * invp[j]
    return q


def statistic(a, ms, nsk, theta=THETA):
    """dict(E [8], form [35], df, q, thr, p, testable) of one gene."""
    E, V = moments(ms, nsk)
    form, df = factor(E, V, max(klast(nsk) - 1, 0), theta)
    q = q_of(a, form)
    return dict(E=E, form=form, df=df, q=q, thr=q * ONE_MINUS_TAU, p=chi2_sf(q, df) if df else 1.0, testable=df > 0)


# ---- the rational reference ----
def moments_exact(ms, nsk, classes=None):
    """(E, V) over the classes ``classes`` (0-based; default: all eight) as Fractions: V the full covariance."""
    ks = list(range(MAX_CLASSES)) if classes is None else list(classes)
    E = [Fraction(0)] * len(ks)
    V = [[Fraction(0)] * len(ks) for _ in ks]
    for m, row in zip(ms, nsk):
        n = sum(row)
        if n == 0:
            continue
        for x, k in enumerate(ks):
            E[x] += Fraction(m * row[k], n)
        if n >= 2:
            c = Fraction(m * (n - m), n * n * (n - 1))
            for x, j in enumerate(ks):
                for y, k in enumerate(ks):
                    V[x][y] += c * ((n * row[j] if j == k else 0) - row[j] * row[k])
    return E, V


def factor_exact(V):
    """(L, pivots, pivots relative to their diagonal: None on a zero diagonal) of the rational LDL' without pivoting;
    under a zero pivot the column is zero (asserted) and stays out of L."""
    n = len(V)
    L = [[Fraction(0)] * n for _ in range(n)]
    piv, rel = [Fraction(0)] * n, []
    for j in range(n):
        p = V[j][j] - sum(L[j][k] * L[j][k] * piv[k] for k in range(j))
        piv[j] = p
        rel.append(p / V[j][j] if V[j][j] else None)
        for i in range(j + 1, n):
            u = V[i][j] - sum(L[i][k] * L[j][k] * piv[k] for k in range(j))
            if p == 0:
                assert u == 0, "a zero pivot over a nonzero column"
            else:
                L[i][j] = u / p
    return L, piv, rel


def q_factored_exact(d, L, piv):
    """(Q = d' V^- d, rank) from factor_exact's L and pivots; a zero pivot must come with a zero contrast (asserted)."""
    n = len(d)
    y, q, rank = [Fraction(0)] * n, Fraction(0), 0
    for j in range(n):
        y[j] = d[j] - sum(L[j][k] * y[k] for k in range(j))
        if piv[j] == 0:
            assert y[j] == 0, "a zero pivot with a nonzero contrast"
            continue
        rank += 1
        q += y[j] * y[j] / piv[j]
    return q, rank


def ldl_exact(d, V):
    """(Q, rank, relative pivots) of one contrast vector."""
    L, piv, rel = factor_exact(V)
    return q_factored_exact(d, L, piv) + (rel,)


def q_exact(a, ms, nsk, drop=None):
    """(Q, rank, relative pivots) in the rationals over all classes but ``drop`` (0-based; default: the last non-empty
    one, the specification's choice; -1: none, the full K x K form)."""
    last = klast(nsk) - 1
    drop = last if drop is None else drop
    ks = [k for k in range(max(last + 1, 0)) if k != drop]
    E, V = moments_exact(ms, nsk, ks)
    return ldl_exact([a[k] - e for k, e in zip(ks, E)], V)


def q_pinv(a, ms, nsk):
    """An independent float route: the full 8 x 8 covariance and numpy's pseudo-inverse."""
    E = np.zeros(MAX_CLASSES)
    V = np.zeros((MAX_CLASSES, MAX_CLASSES))
    for m, row in zip(ms, nsk):
        n = sum(row)
        if n == 0:
            continue
        r = np.array(row, dtype=np.float64)
        E += m * r / n
        if n >= 2:
            V += m * (n - m) / (n * n * (n - 1.0)) * (n * np.diag(r) - np.outer(r, r))
    d = np.array(a[:MAX_CLASSES], dtype=np.float64) - E
    scale = max(float(np.abs(V).max()), 1e-300)
    return float(d @ np.linalg.pinv(V / scale, rcond=1e-10, hermitian=True) @ d) / scale


# ---- the float route over many genes ----
def moments_many(ms, nsk):
    """ms int64 [G, S] -> (E float64 [G, 8], V float64 [G, 7, 7] lower triangle): moments() for every gene."""
    ms = np.asarray(ms, dtype=np.int64)
    G = ms.shape[0]
    E, V = np.zeros((G, MAX_CLASSES)), np.zeros((G, NC, NC))
    for s, row in enumerate(nsk):
        n = sum(row)
        if n == 0:
            continue
        m = ms[:, s]
        for k in range(MAX_CLASSES):
            E[:, k] += (m * row[k]).astype(np.float64) / float(n)
        if n >= 2:
            c = (m.astype(np.float64) * (n - m).astype(np.float64)) / ((float(n) * float(n)) * float(n - 1))
            for j in range(NC):
                for k in range(j + 1):
                    V[:, j, k] += c * float((n * row[j] if j == k else 0) - row[j] * row[k])
    return E, V


def factor_many(E, V, nc, theta=THETA):
    """factor() for every gene: (form float64 [G, 35], df int64 [G])."""
    G = E.shape[0]
    nf = NC * (NC - 1) // 2
    f, invp, df = np.zeros((G, nf)), np.zeros((G, NC)), np.zeros(G, dtype=np.int64)
    u = np.zeros((G, NC, NC))
    zero = np.zeros(G)
    for j in range(NC):
        for k in range(j):
            x = V[:, j, k].copy() if j < nc else zero.copy()
            for l in range(k):
                x = x - u[:, j, l] * f[:, fidx(k, l)]
            u[:, j, k] = x
            f[:, fidx(j, k)] = x * invp[:, k]
        vjj = V[:, j, j] if j < nc else zero
        p = vjj.copy()
        for k in range(j):
            p = p - u[:, j, k] * f[:, fidx(j, k)]
        keep = ~(p <= theta * vjj)
        invp[keep, j] = 1.0 / p[keep]
        df += keep
    Ef = E[:, :NC].copy()
    Ef[:, nc:] = 0.0
    return np.concatenate([Ef, f, invp], axis=1), df


def q_many(a, form):
    """q_of() of counts a [.., G, >= 7] under the forms [G, 35] -> float64 [.., G]."""
    a = np.asarray(a)
    E, f, invp = form[:, :NC], form[:, NC:FORM - NC], form[:, FORM - NC:]
    y = []
    for i in range(NC):
        x = a[..., i].astype(np.float64) - E[:, i]
        for j in range(i):
            x = x - f[:, fidx(i, j)] * y[j]
        y.append(x)
    q = np.zeros(a.shape[:-1])
    for j in range(NC):
        q = q + (y[j] * y[j]) * invp[:, j]
    return q


# ---- permutations ----
def lrow(codes, strata, S):
    """The codes of the valid isolates in (stratum, isolate) order: the generator's d_l."""
    return [c for s in range(S) for c, st in zip(codes, strata) if c and st == s]


def perm_row(seed, t, pi, codes, strata, S):
    """The code row of permutation ``pi`` of trait ``t``: S16's shuffle of the codes within the strata."""
    pl = dict(valid=[1 if c else 0 for c in codes], strata=list(strata), S=S, L=lrow(codes, strata, S))
    return vs.perm_row(seed, t, pi, pl)


def most_enriched(a, E):
    """The index of the class with the largest a_k / E_k over E_k > 0 (fp64 quotients, ties to the first)."""
    best, top = None, -1.0
    for k, (ak, ek) in enumerate(zip(a, E)):
        if ek > 0.0 and float(ak) / ek > top:
            best, top = k, float(ak) / ek
    return best



def clonal_scenario():
    """A clonal population of two lineages of 70 isolates whose label follows the lineage: (genes [3][N] 0/1, labels
    [N] strings, strata [N]).  Gene 0 marks the lineage (and nothing inside it), gene 1 follows the label inside both
    lineages, gene 2 is noise."""
    rng = np.random.default_rng(2021)
    n = 70
    strata = [0] * n + [1] * n
    labels = [("pig", "cattle", "human")[k] for k in
              list(rng.choice(3, n, p=[0.8, 0.1, 0.1])) + list(rng.choice(3, n, p=[0.1, 0.1, 0.8]))]
    marker = [int(rng.random() < (0.93 if s == 0 else 0.07)) for s in strata]
    within = [int(rng.random() < (0.85 if x == "cattle" else 0.15)) for x in labels]
    noise = [int(rng.random() < 0.5) for _ in strata]
    return [marker, within, noise], labels, strata
