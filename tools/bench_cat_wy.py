"""The Westfall-Young kernels of the categorical traits (spec S22) against the plain kernels they extend, at cfg3's
geometry with one trait on one MI355X: G = 50 000 genes (Roary-like frequencies from synth), N = 2000 isolates (or
``isolates``: up to 1280 k_cat_permute fits two blocks on a CU), P = 10 000 label permutations, K = 4 and K = 8
classes, 10 strata for the generalized CMH pair.

Timed, every repeat in the same process after warm-up, the variants alternating inside a repeat, each by device events
(set_timing / kernel_ms):
  * k_cat_maxt (engine.categorical_westfall_young) against k_cat_permute (engine.categorical_permute);
  * k_gcmh_maxt (engine.gcmh_westfall_young) against k_gcmh_permute (engine.gcmh_permute).
Before anything is timed the counts of the fused pass are held to the plain pass's, and r_fwer to r_fwer >= r.
Reported: median, min and max of each and the two ratios with the plain kernel's run-to-run spread -- reported, not
gated: the alternative to the fused pass is a second full pass, a ratio of 2.  Raw lines on stdout
(profiles/cat_wy.txt); every sample on a "raw" line, for an A/B of two builds (SCOARY_HIP_LIB, build_alt.sh:
profiles/cat_block.txt).
    python tools/bench_cat_wy.py [repeats] [warmup] [isolates]"""
import datetime
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from scoary_amd import synth
from scoary_amd.engine import AssociationEngine

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 2
ISOLATES = int(sys.argv[3]) if len(sys.argv) > 3 else None
STRATA = 10
SHARES = {4: [0.4, 0.3, 0.2, 0.1], 8: [0.3, 0.2, 0.15, 0.1, 0.1, 0.05, 0.05, 0.05]}

if not torch.cuda.is_available():
    sys.exit("bench_cat_wy needs an MI355X: there is nothing to time without one")

genes, _traits, P, seed = synth.make_config("cfg3", T=1, N=ISOLATES)
G, N = genes.shape
eng = AssociationEngine(0)
gm = eng.pack_dense(genes)
print("date %s  shape G=%d N=%d T=1 P=%d S=%d  repeats %d warm-up %d  library %s" % (
    datetime.date.today().isoformat(), G, N, P, STRATA, REPEATS, WARMUP, os.environ.get("SCOARY_HIP_LIB", "the tree's")),
    flush=True)


def timed(fn, kernel):
    eng.set_timing(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, eng.kernel_ms(kernel)
    finally:
        eng.set_timing(False)


def line(name, xs):
    print("%-44s median %9.3f ms  min %9.3f  max %9.3f  (n=%d)" % (name, statistics.median(xs), min(xs), max(xs),
                                                                   len(xs)), flush=True)


for K in (4, 8):
    rng = np.random.default_rng(seed + 22 + K)
    codes = rng.choice(np.arange(1, K + 1), size=(1, N), p=SHARES[K])
    codes[0, rng.random(N) < 0.01] = 0
    strata = rng.integers(0, STRATA, N)
    strata[0] = STRATA - 1
    cplan, gplan = eng.categorical_plan(codes), eng.gcmh_plan(codes, strata)
    cobs, gobs = eng.categorical(gm, cplan), eng.gcmh(gm, gplan)
    pairs = {
        "cat": (lambda: eng.categorical_permute(gm, cplan, cobs["a"], P, seed), "k_cat_permute",
                lambda: eng.categorical_westfall_young(gm, cplan, cobs, P, seed), "k_cat_maxt"),
        "gcmh": (lambda: eng.gcmh_permute(gm, gplan, gobs, P, seed), "k_gcmh_permute",
                 lambda: eng.gcmh_westfall_young(gm, gplan, gobs, P, seed), "k_gcmh_maxt"),
    }
    for name, (plain, _pk, fused, _fk) in pairs.items():
        r_plain = plain()
        r, r_fwer, maxs = fused()
        bad = int((r != r_plain).sum())
        print("K=%d %s: the fused pass against the plain one: %d of %d counts differ; r_fwer < r on %d genes; "
              "r_fwer < P on %d genes; maxs from %.4g to %.4g" % (
                  K, name, bad, G, int((r_fwer < r).sum()), int((r_fwer < P).sum()), float(maxs.min()),
                  float(maxs.max())), flush=True)
        if bad or int((r_fwer < r).sum()):
            sys.exit("the counts disagree: nothing is timed")
    t = {k: [] for k in ("k_cat_permute", "k_cat_maxt", "k_gcmh_permute", "k_gcmh_maxt")}
    for i in range(WARMUP + REPEATS):
        for name in (("cat", "gcmh") if i % 2 == 0 else ("gcmh", "cat")):
            plain, pk, fused, fk = pairs[name]
            for fn, kernel in (((plain, pk), (fused, fk)) if i % 2 == 0 else ((fused, fk), (plain, pk))):
                _out, ms = timed(fn, kernel)
                if i >= WARMUP:
                    t[kernel].append(ms)
    for kernel, xs in t.items():
        line("K=%d %s" % (K, kernel), xs)
        print("raw N=%d K=%d %s %s" % (N, K, kernel, " ".join("%.4f" % x for x in xs)), flush=True)
    med = {k: statistics.median(v) for k, v in t.items()}
    for plain, fused in (("k_cat_permute", "k_cat_maxt"), ("k_gcmh_permute", "k_gcmh_maxt")):
        print("K=%d: %s / %s = %.3f (%s's spread %.3f ms, %.1f %% of its median)" % (
            K, fused, plain, med[fused] / med[plain], plain, max(t[plain]) - min(t[plain]),
            100.0 * (max(t[plain]) - min(t[plain])) / med[plain]), flush=True)
try:
    import __graft_entry__ as ge
    with open(ge.HIP_RESOURCES) as f:
        res = json.load(f)
    for name, fields in res.items():
        for kernel in ("k_cat_permute", "k_cat_maxt", "k_gcmh_permute", "k_gcmh_maxt"):
            if kernel in name:
                print("%s resources: " % kernel + ", ".join("%s %s" % kv for kv in sorted(fields.items())), flush=True)
except (OSError, ImportError, ValueError):
    print("kernel resources: the build's report was not found", flush=True)
