"""The problems of tests/test_gpu_score_spa.py, made on the host (a helper, not a test), so that the CPU tests can hold
the restatement of S25 to them too: the shapes, the traits and genes of a shape, S24's outputs for them by the
restatement of S24 (score_spec), and the restatement of S25 (score_spa_spec) over every pair."""
import math

import numpy as np

import score_spa_spec as sp
import score_spec as ss

# name: (N, G, covariates); T = 3 everywhere: trait 0 balanced, trait 1 in one class (S24 skips it: an empty valid
# set), trait 2 rare -- 5 % positives at N = 600, 6 % (8 isolates) at N = 130, about 30 % where fewer isolates leave
# no null model at 5 %.  N: fewer isolates than lanes; a word edge (64, 65); invalid isolates in the middle of a row
# (every trait misses isolates of its own); three words and a tail (130); ten strides of the lanes (600).
# G = 300 with T = 3 is more pairs than wavefronts are launched for: the list is walked in strides.
SHAPES = {
    "n7": (7, 1, 0),
    "n64": (64, 300, 2),
    "n65": (65, 70, 8),
    "n130": (130, 70, 2),
    "n600": (600, 70, 2),
}
T = 3
RARE = {7: 2.0 / 7, 64: 0.3, 65: 0.3, 130: 0.06, 600: 0.05}
# The least cutoff, 0.1, sends rows to the saddlepoint that no run would: about one pair in 200 of such problems then
# falls back by S25's own rule (a rare gene in a rare trait whose statistic is far below 1: the correction term
# log(v / omega) / omega outweighs omega and z changes sign).  What the sides leave at status 2 is not specified, so
# the device is held to z and t^ on problems without one: a seed per shape at which the restatement never falls back,
# and in the shapes with a 5 % trait the carriers of the one- and two-carrier genes have no value in that trait (with
# one, such a gene without a positive carrier is the pair that falls back: statistic 0.03 to 0.08).
# test_score_spa_spec.py holds the restatement to "no status 2" on exactly these problems.  fallback_problem() is the
# one made the other way, n130 with those values kept: two of its pairs fall back, and the device is held to the
# status and the p of every pair of it, not to z and t^.
SEEDS = {"n7": 2503, "n64": 2503, "n65": 2503, "n130": 2505, "n600": 2505}


def problem(name, fallbacks=False):
    """(genes [G, N] 0/1, values [T, N], covariates [c, N]) of a shape.  Covariate 0 is 0 / 1.  The single gene of
    n7 is trait 0 itself.  In a shape with G >= 70 the first genes belong to the rare trait 2 -- three rare genes
    carried by most of its positives and by one or two other isolates in a hundred, and trait 2 itself (perfectly
    predictive at a small mu) -- and the last genes to trait 0: one carrier, two, all but one of its valid isolates,
    trait 0 itself (perfectly predictive), and covariate 0 (in the span of the covariates: untestable).
    ``fallbacks``: see fallback_problem."""
    N, G, c = SHAPES[name]
    rng = np.random.default_rng(SEEDS[name] + sum(map(ord, name)))
    cov = rng.standard_normal((c, N))
    if c:
        cov[0] = rng.random(N) < 0.4
        cov[c - 1, N // 3] = np.nan
    values = np.empty((T, N))
    values[0] = np.arange(N) % 2 if N < 10 else rng.random(N) < 0.5
    values[1] = 1.0
    rare = max(2, int(round(RARE[N] * N)))
    values[2] = 0.0
    values[2, rng.permutation(N)[:rare]] = 1.0
    if N >= 64:
        for t in range(T):
            values[t, rng.random(N) < 0.06] = np.nan
            values[t, 20 + t] = np.nan               # invalid isolates in the middle of the first word
    genes = (rng.random((G, N)) < rng.uniform(0.03, 0.6, (G, 1))).astype(np.uint8)
    if G == 1:
        genes[0] = values[0]
    if G >= 70:
        positive = np.nan_to_num(values[2]) == 1.0
        for g in range(3):
            genes[g] = np.where(positive, rng.random(N) < 0.7, rng.random(N) < 0.015)
        genes[3] = positive
        ok = ~np.isnan(values[0]) & ~np.isnan(cov).any(axis=0)
        v0 = np.flatnonzero(ok)
        one, two, most = np.zeros(N), np.zeros(N), ok.astype(float)
        one[v0[3]] = 1
        two[v0[[1, -1]]] = 1
        most[v0[5]] = 0
        if RARE[N] < 0.1 and not fallbacks:
            values[2, v0[[1, 3, -1]]] = np.nan
        special = [one, two, most, np.nan_to_num(values[0]), cov[0] == 1.0]
        for k, row in enumerate(special):
            genes[G - 1 - k] = row
    return genes, values, cov


def fallback_problem():
    """n130 with the values of trait 2 kept at the carriers of the one- and two-carrier genes: two pairs fall back at
    the least cutoff."""
    return problem("n130", fallbacks=True)


def s24(host, genes):
    """S24's outputs for every (trait, gene) by its restatement on the host plan's rows: dict of arrays U, Vg, stat,
    p [T, G], b [T, G, q], testable [T, G]."""
    Tn, rows_n, N = host["rows"].shape
    G, q = len(genes), rows_n - 1
    out = dict(U=np.zeros((Tn, G)), Vg=np.zeros((Tn, G)), stat=np.zeros((Tn, G)), p=np.ones((Tn, G)),
               b=np.zeros((Tn, G, q)), testable=np.zeros((Tn, G), dtype=bool))
    for t in range(Tn):
        rows = [r.tolist() for r in host["rows"][t]]
        valid = host["valid"][t].astype(int).tolist()
        packed = host["chol"][t].tolist()
        for g in range(G):
            r = ss.statistic(genes[g].tolist(), rows, valid, packed, "logistic")
            out["U"][t, g], out["Vg"][t, g], out["stat"][t, g] = r["U"], r["Vg"], r["stat"]
            out["b"][t, g] = r["b"]
            out["testable"][t, g] = r["testable"]
            out["p"][t, g] = ss.p_of("logistic", r["stat"], r["df"], r["testable"])
    return out


def restate(spa_rows, weights, valid, chol, genes, score, cutoff):
    """The restatement of S25 over every (trait, gene): spa_rows [T, q + 1, N], weights [T, N] (row 1 of S24's rows),
    valid bool [T, N], chol [T, q (q + 1) / 2], score = dict of S24's outputs (U, b, Vg, stat, p as arrays).  Returns
    [T][G] dicts as score_spa_spec.spa gives them."""
    Tn = len(spa_rows)
    out = []
    for t in range(Tn):
        rows = [r.tolist() for r in spa_rows[t]]
        w, v, packed = weights[t].tolist(), valid[t].astype(int).tolist(), chol[t].tolist()
        out.append([sp.spa(genes[g].tolist(), rows, w, v, packed, float(score["U"][t, g]), score["b"][t, g].tolist(),
                           float(score["Vg"][t, g]), float(score["stat"][t, g]), float(score["p"][t, g]), cutoff)
                    for g in range(len(genes))])
    return out


def at_cutoff(every, score, cutoff):
    """What restate gives at ``cutoff`` from what it gave at the least cutoff: a pair at or above the cutoff does not
    depend on it, a pair below is status 0 with S24's p."""
    c2 = cutoff * cutoff
    return [[r if not score["stat"][t, g] < c2 else dict(p=float(score["p"][t, g]), z=[0.0, 0.0], t=[0.0, 0.0],
                                                         status=0)
             for g, r in enumerate(row)] for t, row in enumerate(every)]


def normal_tail(z):
    return 0.5 * math.erfc(abs(z) / math.sqrt(2.0))
