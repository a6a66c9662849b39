"""The saddlepoint-corrected p of the logistic score test (spec S25) at the headline shape on one MI355X: G = 50 000
genes (Roary-like frequencies from synth), N = 2000 isolates, T = 10 traits, c = 4 covariates, with a balanced trait
set and one at 5 % positives.

Timed by device events (set_timing / kernel_ms), every repeat in the same process, the variants alternating inside a
repeat:
  * scoary_score_spa (its four kernels: the select pass, the search, the sums at the roots, the finish) at the default
    cutoff 2 and at the least, 0.1, where the work list holds every testable pair;
  * k_score_observed, S24's own pass over the same plan, in the same run.
Reported: median, min and max of each, the work-list sizes, the statuses, the ratio to k_score_observed, and the search's
(isolate, evaluation) terms per second at cutoff 0.1 under an assumed 2 x 8 evaluations a pair.  Raw lines on stdout
(profiles/score_spa.txt).
    python tools/bench_score_spa.py [repeats] [warmup]"""
import datetime
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from scoary_amd import synth
from scoary_amd.engine import AssociationEngine, score_host

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 1
T, C = 10, 4

if not torch.cuda.is_available():
    sys.exit("bench_score_spa needs an MI355X: there is nothing to time without one")
genes, _traits, _P, seed = synth.make_config("cfg3", T=1)
G, N = genes.shape
rng = np.random.default_rng(seed + 25)
cov = rng.standard_normal((C, N))
eta = cov.T @ rng.standard_normal(C) / 2.0
lo, hi = -10.0, 0.0                                   # the intercept at which 5 % of the isolates are positive
for _ in range(60):
    mid = 0.5 * (lo + hi)
    lo, hi = (mid, hi) if (1.0 / (1.0 + np.exp(-(eta + mid)))).mean() < 0.05 else (lo, mid)
traits = {"balanced": (rng.random((T, N)) < 1.0 / (1.0 + np.exp(-eta[None, :]))).astype(np.float64),
          "5 % positives": (rng.random((T, N)) < 1.0 / (1.0 + np.exp(-(eta[None, :] + lo)))).astype(np.float64)}
eng = AssociationEngine(0)
gm = eng.pack_dense(genes)
print("date %s  shape G=%d N=%d T=%d c=%d  repeats %d warm-up %d" % (datetime.date.today().isoformat(), G, N, T, C,
                                                                      REPEATS, WARMUP), flush=True)


def timed(fn, kernel):
    eng.set_timing(True)
    try:
        fn()
        torch.cuda.synchronize()
        return eng.kernel_ms(kernel)
    finally:
        eng.set_timing(False)


for label, values in traits.items():
    plan = eng.score_plan_of(score_host(values, cov, "logistic"), "logistic")
    assert plan.skipped == [None] * T, plan.skipped
    score = eng.score(gm, plan)
    print("%s: %.1f %% positives, %d of %d pairs testable" % (label, 100.0 * values.mean(), int((score["p"] < 1.0).sum()),
                                                               T * G), flush=True)
    variants = [("k_score_observed", lambda: eng.score(gm, plan), "k_score_observed")]
    sizes = {}
    for cutoff in (2.0, 0.1):
        out = eng.score_spa(gm, plan, score, cutoff)
        status = out["status"].cpu().numpy()
        sizes[cutoff] = int((status != 0).sum())
        ratio = (out["p"] / score["p"])[out["status"] == 1]
        print("%s cutoff %.1f: work list %d pairs, status 1 %d, status 2 %d; SPA_p / Score_p over status 1: median "
              "%.3g, max %.3g" % (label, cutoff, sizes[cutoff], int((status == 1).sum()), int((status == 2).sum()),
                                  float(ratio.median()), float(ratio.max())), flush=True)
        variants.append(("scoary_score_spa cutoff %.1f" % cutoff,
                         (lambda c=cutoff: eng.score_spa(gm, plan, score, c)), "k_score_spa"))
    t = {name: [] for name, _fn, _k in variants}
    for i in range(WARMUP + REPEATS):
        for name, fn, kernel in (variants if i % 2 == 0 else variants[::-1]):
            ms = timed(fn, kernel)
            if i >= WARMUP:
                t[name].append(ms)
    base = statistics.median(t["k_score_observed"])
    for name, xs in t.items():
        print("%s: %-32s median %9.3f ms  min %9.3f  max %9.3f  (n=%d)  %.2f x k_score_observed"
              % (label, name, statistics.median(xs), min(xs), max(xs), len(xs), statistics.median(xs) / base), flush=True)
    ms = statistics.median(t["scoary_score_spa cutoff 0.1"])
    print("%s: cutoff 0.1: %.3g (isolate, evaluation) terms per second if a pair takes 2 x 8 evaluations"
          % (label, sizes[0.1] * 16.0 * N / (ms * 1e-3)), flush=True)
try:
    import __graft_entry__ as ge
    with open(ge.HIP_RESOURCES) as f:
        res = json.load(f)
    for name, fields in sorted(res.items()):
        if "k_score_spa" in name or "k_spa_" in name:
            print("%s: VGPRs %s, SGPRs %s, scratch %s" % (name[:44], fields.get("VGPRs"), fields.get("TotalSGPRs"),
                                                         fields.get("ScratchSize")), flush=True)
except (OSError, ImportError, ValueError):
    print("kernel resources: the build's report was not found", flush=True)
