"""The exact conditional odds ratio and its confidence limits (spec S13) at cfg3's shape on one MI355X: k_cmh_odds_exact
beside k_cmh_exact (set_timing / kernel_ms) for S = 50 and S = 256 strata, assigned at random (interleaved) and in
index blocks (contiguous), timed in one process with the two kernels and the four variants alternating inside every
repeat.  A sample of (trait, gene) pairs per variant is also solved on the host by the kernel's own iteration in numpy
(solve(), below): it counts the Newton iterations a row takes -- the kernel has one barrier per iteration -- and its
values are compared with the device's.  Raw lines on stdout (profiles/cmh_exact_odds.txt).
    python tools/cmh_exact_odds_bench.py [repeats] [sampled pairs per variant]"""
import math, os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from scoary_amd import synth
from scoary_amd.engine import AssociationEngine, pack_bits_rows

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
SAMPLE = int(sys.argv[2]) if len(sys.argv) > 2 else 150
LEVEL = 0.95


def stratum_pmf(m, k, n):
    """S12 step 1: the hypergeometric pmf on [max(0, k + m - n), min(k, m)] by the ratio recurrence from the mode."""
    lo, hi = max(0, k + m - n), min(k, m)
    xm = min(max(((m + 1) * (k + 1)) // (n + 2), lo), hi)
    f = np.zeros(hi - lo + 1)
    f[xm - lo] = w = 1.0
    for x in range(xm, hi):
        w = (w * (float(m - x) * float(k - x))) / (float(x + 1) * float(n - m - k + x + 1))
        f[x + 1 - lo] = w
    w = 1.0
    for x in range(xm, lo, -1):
        w = (w * (float(x) * float(n - m - k + x))) / (float(m - x + 1) * float(k - x + 1))
        f[x - 1 - lo] = w
    return lo, f / f.sum()


def solve(f, xa, half):
    """k_cmh_odds_exact's iteration in numpy: (odds, lower, upper, iterations)."""
    L = len(f)
    if L == 1:
        return math.nan, 0.0, math.inf, 0
    with np.errstate(divide="ignore"):
        lf = np.log(f / (f[xa] if f[xa] >= 1e-290 else 1.0))
    x = np.arange(L) - float(xa)
    target = math.log(half) - math.log1p(-half)
    roots = [dict(th=0.0, lo=-700.0, hi=700.0, done=d) for d in (not 0 < xa < L - 1, not xa > 0, not xa < L - 1)]
    sides = [(x > 0, np.abs(x), 0.0), (x >= 0, 1.0, -target), (x > 0, 1.0, target)]        # (upper side, weight, shift)
    it = 0
    while it < 128 and not all(r["done"] for r in roots):
        it += 1
        for r, (up, c, shift) in zip(roots, sides):
            if r["done"]:
                continue
            e = lf + r["th"] * x
            w = np.exp(e - e.max()) * c
            with np.errstate(all="ignore"):
                U, D, U1, D1 = w[up].sum(), w[~up].sum(), (w * x)[up].sum(), (w * x)[~up].sum()
                h, dh = np.log(U) - np.log(D) + shift, U1 / U - D1 / D
                if h > 0:
                    r["hi"] = r["th"]
                elif h < 0:
                    r["lo"] = r["th"]
                dn = -h / dh
            small, nt = abs(dn) < 1e-13, r["th"] + dn
            if not r["lo"] < nt < r["hi"]:
                nt = r["th"] if small else 0.5 * (r["lo"] + r["hi"])
            r["done"] = bool(small or abs(nt - r["th"]) < 1e-13 or r["hi"] - r["lo"] < 1e-13)
            r["th"] = float(nt)
    psi = [0.0 if r["th"] <= -700 + 1e-9 else (math.inf if r["th"] >= 700 - 1e-9 else math.exp(r["th"])) for r in roots]
    return (0.0 if xa == 0 else (math.inf if xa == L - 1 else psi[0]), 0.0 if xa == 0 else psi[1],
            math.inf if xa == L - 1 else psi[2], it)


def host_sample(genes, traits, strata, S, got, count, rng):
    """``count`` random pairs on the host: (iterations per row, the largest relative difference to the device)."""
    its, worst = [], 0.0
    for _ in range(count):
        t, g = int(rng.integers(traits.shape[0])), int(rng.integers(genes.shape[0]))
        valid, lab, gene = traits[t] != 2, traits[t] == 1, genes[g] == 1
        n, k = np.bincount(strata[valid], minlength=S), np.bincount(strata[lab], minlength=S)
        m, a = np.bincount(strata[valid & gene], minlength=S), np.bincount(strata[lab & gene], minlength=S)
        f, lo = np.ones(1), 0
        for s in range(S):
            if n[s] > 0:
                lo_s, fs = stratum_pmf(int(m[s]), int(k[s]), int(n[s]))
                lo += lo_s
                if len(fs) > 1:
                    f = np.convolve(f, fs)
        want = solve(f, int(a[n > 0].sum()) - lo, 0.5 * (1.0 - LEVEL))
        its.append(want[3])
        for w, v in zip(want[:3], got[:, t, g]):
            if math.isfinite(w) and w > 0:
                worst = max(worst, abs(float(v) - w) / w)
            else:
                assert v == w or (math.isnan(w) and math.isnan(v)), (t, g, w, v)
    return its, worst


genes, traits, P, seed = synth.make_config("cfg3")
G, N = genes.shape; T = traits.shape[0]
eng = AssociationEngine(0)
gm = eng.pack_dense(genes)
trv = eng.vecrows(pack_bits_rows((traits == 1).astype(np.uint8)), N)
mkv = eng.vecrows(pack_bits_rows((traits != 2).astype(np.uint8)), N)
print("shape G=%d N=%d T=%d repeats %d level %s" % (G, N, T, REPEATS, LEVEL), flush=True)

rng = np.random.default_rng(1)
layouts = [("S=50 interleaved", rng.integers(0, 50, N), 50), ("S=50 contiguous", np.arange(N) * 50 // N, 50),
           ("S=256 interleaved", rng.integers(0, 256, N), 256), ("S=256 contiguous", np.arange(N) * 256 // N, 256)]
variants = [(name, eng.strata_plan(strata, trv, mkv, N, S=S)) for name, strata, S in layouts]


def timed(name, fn):
    eng.set_timing(True)
    try:
        out = fn()
        return out, eng.kernel_ms(name)
    finally:
        eng.set_timing(False)


cm = {name: eng.cmh(gm, trv, mkv, sp) for name, sp in variants}
runs = {"exact": ("k_cmh_exact", lambda n, sp: eng.cmh_exact(gm, mkv, sp, cm[n])),
        "exact odds": ("k_cmh_odds_exact", lambda n, sp: eng.cmh_exact_odds(gm, mkv, sp, cm[n], level=LEVEL))}
for (name, sp), (_name, strata, S) in zip(variants, layouts):
    od = runs["exact odds"][1](name, sp)
    got = np.stack([od[k].cpu().numpy() for k in ("odds", "lower", "upper")])
    its, worst = host_sample(genes, traits, np.asarray(strata), S, got, SAMPLE, np.random.default_rng(S))
    print("%-18s %d sampled pairs: Newton iterations (= barriers of the solver) per row mean %.2f, median %d, max %d; "
          "device against the host's run of the same iteration: max relative difference %.2e; nan %d, 0 %d, inf %d of "
          "%d odds" % (name, SAMPLE, statistics.mean(its), statistics.median(its), max(its), worst,
                       int(np.isnan(got[0]).sum()), int((got[0] == 0).sum()), int(np.isinf(got[0]).sum()), T * G),
          flush=True)
    runs["exact"][1](name, sp)
torch.cuda.synchronize()
ms = {(name, kind): [] for name, _ in variants for kind in runs}
for i in range(REPEATS):
    for name, sp in (variants if i % 2 == 0 else variants[::-1]):
        for kind in (list(runs) if i % 2 == 0 else list(runs)[::-1]):
            out, got_ms = timed(runs[kind][0], lambda: runs[kind][1](name, sp))
            ms[(name, kind)].append(got_ms)
            del out
for name, _sp in variants:
    for kind in runs:
        v = ms[(name, kind)]
        print("%-18s %-11s %-17s median %.3f ms (min %.3f max %.3f)"
              % (name, kind, runs[kind][0], statistics.median(v), min(v), max(v)), flush=True)
