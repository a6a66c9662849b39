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
# n97 .. n199: one shape for each of 1, 3, 4, 5, 6 and 7 covariates, so that with the others every instance q = 1 .. 9
# of the search and of the sums runs (from q = 4 on the rows are reached through one running address); 5 % positives
# in trait 2 at each of them.  n4099: 65 strides of the lanes with a short last one, a word tail and a tail of the
# tiled matrix's groups of four words; n65536: scoary_score_spa_max_isolates() itself, 1024 isolates a lane.  The
# restatement of these two over every pair takes minutes, so the tests restate the pairs of LISTED alone (SUBSET).
SHAPES = {
    "n7": (7, 1, 0),
    "n64": (64, 300, 2),
    "n65": (65, 70, 8),
    "n130": (130, 70, 2),
    "n600": (600, 70, 2),
    "n97": (97, 70, 1),
    "n113": (113, 70, 3),
    "n128": (128, 70, 4),
    "n150": (150, 70, 5),
    "n177": (177, 70, 6),
    "n199": (199, 70, 7),
    "n4099": (4099, 70, 2),
    "n65536": (65536, 4, 1),
}
SUBSET = ("n4099", "n65536")
EVERY_PAIR = tuple(name for name in SHAPES if name not in SUBSET)      # restated over every pair
T = 3
RARE = {7: 2.0 / 7, 64: 0.3, 65: 0.3, 130: 0.06, 600: 0.05, 97: 0.05, 113: 0.05, 128: 0.05, 150: 0.05, 177: 0.05,
        199: 0.05, 4099: 0.05, 65536: 0.05}
# The least cutoff, 0.1, sends rows to the saddlepoint that no run would: about one pair in 200 of such problems then
# falls back by S25's own rule (a rare gene in a rare trait whose statistic is far below 1: the correction term
# log(v / omega) / omega outweighs omega and z changes sign).  What the sides leave at status 2 is not specified, so
# the device is held to z and t^ on problems without one: a seed per shape at which the restatement never falls back,
# and in the shapes with a 5 % trait the carriers of the one- and two-carrier genes have no value in that trait (with
# one, such a gene without a positive carrier is the pair that falls back: statistic 0.03 to 0.08).
# test_score_spa_spec.py holds the restatement to "no status 2" on exactly these problems.  fallback_problem() is the
# one made the other way, n130 with those values kept: two of its pairs fall back, and the device is held to the
# status and the p of every pair of it, not to z and t^.
SEEDS = {"n7": 2503, "n64": 2503, "n65": 2503, "n130": 2505, "n600": 2505, "n97": 2552, "n113": 2513, "n128": 2506,
         "n150": 2503, "n177": 2504, "n199": 2503, "n4099": 2503, "n65536": 2503}
# The pairs of a SUBSET shape that the tests list (through fabricate) and restate, each found to have status 1.
# n4099: the three rare genes of trait 2 and trait 2 itself (a point mass that underflows to 0 above, 56 evaluations
# below), the perfectly predictive gene of trait 0 (a point mass and a side beyond the support), its two-carrier and
# all-but-one genes, and five ordinary pairs whose searches take 13 to 42 evaluations.  (Over every pair n4099 has
# one status 2 at the least cutoff at this seed, the one-carrier gene of trait 0, and one or two at each of the 14
# other seeds that were tried, always that gene or the all-but-one gene: a statistic of about 1 on a lattice of one
# step.  It is not listed.)
LISTED = {
    "n4099": ((2, 0), (2, 1), (2, 2), (2, 3), (0, 66), (0, 68), (0, 67), (0, 15), (0, 53), (2, 12), (2, 37), (0, 16)),
    "n65536": ((0, 1), (2, 3)),
}


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


def ends_problem():
    """n130 with one more gene, the last: 1 - trait 0 on trait 0's valid set, perfectly anti-predictive (U < 0, -|U|
    at the lower end of the support: the point mass of side 1, and +|U| beyond the upper end)."""
    genes, values, cov = problem("n130")
    ok = ~np.isnan(values[0]) & ~np.isnan(cov).any(axis=0)
    anti = np.where(ok, 1.0 - np.nan_to_num(values[0]), 0.0).astype(np.uint8)
    return np.concatenate([genes, anti[None, :]]), values, cov


ENDS_K = (3.0, 0.5, -0.5)           # U = s_end (1 + k 1e-9): beyond the support, and the point mass from both sides
ENDS_DELTA = (1e-2, 1e-4)           # U = s_end (1 - delta): a root close to the end
ENDS_PER_DELTA = 4                  # candidate pairs for each delta and side, of which at least two must be kept


def ends_moves(spa_rows, weights, valid, chol, genes, score):
    """The pairs of ends_problem whose U is moved to an end of their support, from S24's outputs ``score``: ordinary
    testable pairs of trait 0 (genes 4 onwards, in order), for side 0 and then for side 1 three pairs for ENDS_K and
    ENDS_PER_DELTA pairs for each of ENDS_DELTA.  A pair near an end is kept only if device_search ends within 80
    evaluations on both of its sides and the restatement gives status 1.  Returns (U = {(t, g): value} for fabricate,
    what = {(t, g): (side, "k" or "delta", k or delta)}); the sign of a pair's U is kept."""
    ordinary = [g for g in range(4, len(genes) - 6) if float(score["stat"][0, g]) >= sp.MIN_CUTOFF ** 2]
    per_side = len(ENDS_K) + ENDS_PER_DELTA * len(ENDS_DELTA)
    assert len(ordinary) >= 2 * per_side
    U, what = {}, {}
    for side in (0, 1):
        mine = ordinary[side * per_side:(side + 1) * per_side]
        plan = [("k", k) for k in ENDS_K] + [("delta", d) for d in ENDS_DELTA for _ in range(ENDS_PER_DELTA)]
        for g, (kind, v) in zip(mine, plan):
            items = items_of(spa_rows, weights, valid, chol, genes, score, 0, g)
            x = end_of(items, side) * (1.0 + v * 1e-9 if kind == "k" else 1.0 - v)
            value = -x if float(score["U"][0, g]) < 0.0 else x
            if kind == "delta":
                searches = [device_search(items, ax, float(score["Vg"][0, g]), sd) for sd, ax, _e in searched_sides(items, x)]
                r = sp.spa(genes[g].tolist(), [r.tolist() for r in spa_rows[0]], weights[0].tolist(),
                           valid[0].astype(int).tolist(), chol[0].tolist(), value, score["b"][0, g].tolist(),
                           float(score["Vg"][0, g]), 1e6, float(score["p"][0, g]), sp.MIN_CUTOFF)
                if r["status"] != 1 or any(root is None or evals > 80 for root, evals, _u in searches):
                    continue
            U[0, g], what[0, g] = value, (side, kind, v)
    return U, what


WIDE = (40, 175000, 3)              # N, G, T of wide_problem: no covariate
WIDE_SEED = 2503


def wide_problem():
    """525 000 pairs, one more grid-stride of k_spa_select than its 2048 blocks of 256 cover: (genes [G, 40], values
    [3, 40], None).  Three traits of their own (a half, a third and a fifth positive, each without a value at two
    isolates of its own), genes drawn at once."""
    N, G, Tn = WIDE
    rng = np.random.default_rng(WIDE_SEED)
    values = np.stack([(rng.random(N) < share).astype(np.float64) for share in (0.5, 0.35, 0.2)])
    for t in range(Tn):
        values[t, [3 + t, 30 + t]] = np.nan
    genes = (rng.random((G, N)) < rng.uniform(0.1, 0.6, (G, 1))).astype(np.uint8)
    return genes, values, None


def wide_fixed():
    """The pairs of wide_problem that are always listed, as (t, g): pair 0, the last pair, two on each side of pair
    524 288 = 2048 * 256, and ten neighbours."""
    N, G, Tn = WIDE
    at = [0, Tn * G - 1, 524286, 524287, 524288, 524289] + list(range(262144, 262154))
    return [divmod(o, G) for o in at]


def wide_candidates(count=64):
    """The pairs wide_listed chooses from: a CPU test needs S24's outputs of these alone."""
    N, G, Tn = WIDE
    return wide_fixed() + [divmod(o, G) for o in
                           np.random.default_rng(WIDE_SEED + 1).permutation(Tn * G)[:4 * count].tolist()]


def wide_listed(stat, count=64):
    """wide_fixed and, up to ``count``, the first pairs of a fixed random order whose real statistic ``stat`` [T, G]
    is at least 1 (where no pair of these problems falls back)."""
    N, G, Tn = WIDE
    out = wide_fixed()
    for pair in wide_candidates(count)[len(out):]:
        if len(out) < count and stat[pair] >= 1.0 and pair not in out:
            out.append(pair)
    assert len(out) == count
    return out


def s24(host, genes, pairs=None):
    """S24's outputs for every (trait, gene) by its restatement on the host plan's rows: dict of arrays U, Vg, stat,
    p [T, G], b [T, G, q], testable [T, G].  ``pairs``: only those (trait, gene) are computed, every other cell is
    that of an untestable gene."""
    Tn, rows_n, N = host["rows"].shape
    G, q = len(genes), rows_n - 1
    out = dict(U=np.zeros((Tn, G)), Vg=np.zeros((Tn, G)), stat=np.zeros((Tn, G)), p=np.ones((Tn, G)),
               b=np.zeros((Tn, G, q)), testable=np.zeros((Tn, G), dtype=bool))
    for t in range(Tn):
        wanted = range(G) if pairs is None else sorted({g for tt, g in pairs if tt == t})
        if not len(wanted):
            continue
        rows = [r.tolist() for r in host["rows"][t]]
        valid = host["valid"][t].astype(int).tolist()
        packed = host["chol"][t].tolist()
        for g in wanted:
            r = ss.statistic(genes[g].tolist(), rows, valid, packed, "logistic")
            out["U"][t, g], out["Vg"][t, g], out["stat"][t, g] = r["U"], r["Vg"], r["stat"]
            out["b"][t, g] = r["b"]
            out["testable"][t, g] = r["testable"]
            out["p"][t, g] = ss.p_of("logistic", r["stat"], r["df"], r["testable"])
    return out


def restate(spa_rows, weights, valid, chol, genes, score, cutoff, pairs=None):
    """The restatement of S25 over every (trait, gene): spa_rows [T, q + 1, N], weights [T, N] (row 1 of S24's rows),
    valid bool [T, N], chol [T, q (q + 1) / 2], score = dict of S24's outputs (U, b, Vg, stat, p as arrays).  Returns
    [T][G] dicts as score_spa_spec.spa gives them; with ``pairs``, a dict {(trait, gene): that dict} of those alone."""
    Tn = len(spa_rows)
    out = {} if pairs is not None else []
    for t in range(Tn):
        wanted = range(len(genes)) if pairs is None else sorted({g for tt, g in pairs if tt == t})
        if not len(wanted):
            continue
        rows = [r.tolist() for r in spa_rows[t]]
        w, v, packed = weights[t].tolist(), valid[t].astype(int).tolist(), chol[t].tolist()
        row = [sp.spa(genes[g].tolist(), rows, w, v, packed, float(score["U"][t, g]), score["b"][t, g].tolist(),
                      float(score["Vg"][t, g]), float(score["stat"][t, g]), float(score["p"][t, g]), cutoff)
               for g in wanted]
        if pairs is None:
            out.append(row)
        else:
            out.update(((t, g), r) for g, r in zip(wanted, row))
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


# S25 "The search (device)": the step at which it ends, its cap, and the names of its five rules
DEVICE_STEP = 1e-11
DEVICE_MAX_EVALS = 100
NEWTON_OPEN, GROW_4T, CUT_4T, NEWTON, MIDPOINT = "Newton open", "4t: bad step", "cut to 4t", "Newton bracketed", "midpoint"
RULES = (NEWTON_OPEN, GROW_4T, CUT_4T, NEWTON, MIDPOINT)


def device_search(items, x, Vg, side, max_evals=DEVICE_MAX_EVALS):
    """The device's search of S25 stated from DESIGN.md ("The search (device)"), with the sums by math.fsum: x = |U|,
    side 0 (the root of K'(t) = x) or 1 (of K'(t) = -x), in the side's own coordinates, where the root is positive.
    Newton steps from x / Vg inside a bracket that starts as (0, inf); after every evaluation the bracket end on the
    side of K' - x moves to t; a step that leaves the bracket is replaced by the midpoint, or by 4t while the far
    end is inf, and a step beyond 4t is cut to 4t; the search ends when an applied step is at most 1e-11 relative.
    Returns (t^ with the side's sign, or None at the cap; evaluations; the set of rules that were applied)."""
    sg = -1.0 if side else 1.0
    lo, hi, t = 0.0, math.inf, x / Vg
    used = set()
    for ev in range(1, max_evals + 1):
        _k, k1, k2 = sp.cgf(items, sg * t, with_k=False)
        f = sg * k1 - x
        if f > 0.0:
            hi = t
        else:
            lo = t
        tn = t - f / k2 if k2 != 0.0 else (math.nan if f == 0.0 else math.copysign(math.inf, -f))
        if hi == math.inf:
            if not tn > lo:
                tn, rule = 4.0 * t, GROW_4T
            elif not tn <= 4.0 * t:
                tn, rule = 4.0 * t, CUT_4T
            else:
                rule = NEWTON_OPEN
        elif not (tn > lo and tn < hi):
            tn, rule = 0.5 * (lo + hi), MIDPOINT
        else:
            rule = NEWTON
        used.add(rule)
        if abs(tn - t) <= DEVICE_STEP * abs(tn):
            return sg * tn, ev, used
        t = tn
    return None, max_evals, used


def items_of(spa_rows, weights, valid, chol, genes, score, t, g):
    """score_spa_spec.projected for the pair (t, g) of a problem given as restate takes it."""
    return sp.projected(genes[g].tolist(), [r.tolist() for r in spa_rows[t]], weights[t].tolist(),
                        valid[t].astype(int).tolist(), chol[t].tolist(), score["b"][t, g].tolist())


def searched_sides(items, U):
    """The sides of a listed pair that reach the search: [(side, x, the side's end of the support)], x = |U|."""
    s_lo, s_hi = sp.support(items)
    x = abs(U)
    return [(side, x, end) for side, end in ((0, s_hi), (1, -s_lo))
            if not x > end * (1.0 + sp.EDGE) and not abs(x - end) <= sp.EDGE * end]


def census(spa_rows, weights, valid, chol, genes, score, pairs, every):
    """device_search over every searched side of ``pairs``: [(t, g, side, evaluations, rules, the restatement's
    status of the pair, device_search's root)], ``every`` the restatement as restate gives it ([T][G], or the dict of
    a subset)."""
    out = []
    for t, g in pairs:
        items = items_of(spa_rows, weights, valid, chol, genes, score, t, g)
        for side, x, _end in searched_sides(items, float(score["U"][t, g])):
            root, evals, used = device_search(items, x, float(score["Vg"][t, g]), side)
            status = every[t, g]["status"] if isinstance(every, dict) else every[t][g]["status"]
            out.append((t, g, side, evals, used, status, root))
    return out


def fabricate(score, pairs, U=None):
    """A copy of S24's outputs (arrays) in which stat is 0 everywhere except at ``pairs``, where it is 1e6: the device
    lists exactly those at any cutoff.  U, b, Vg and p are kept, except that ``U`` = {(t, g): value} overwrites U
    there (an end of the pair's support times a chosen factor: see end_of)."""
    out = {k: np.array(v, copy=True) for k, v in score.items()}
    out["stat"][...] = 0.0
    for t, g in pairs:
        out["stat"][t, g] = 1e6
    for (t, g), value in (U or {}).items():
        assert out["stat"][t, g] == 1e6
        out["U"][t, g] = value
    return out


def end_of(items, side):
    """s_hi (side 0) or -s_lo (side 1) of score_spa_spec.support: what x = |U| is compared with on that side."""
    s_lo, s_hi = sp.support(items)
    return -s_lo if side else s_hi
