"""The covariate-adjusted score tests (spec S24) at the headline shape on one MI355X: G = 50 000 genes (Roary-like
frequencies from synth), N = 2000 isolates, T = 10 traits, with c = 4 and c = 8 covariates, both kinds.

Timed by device events (set_timing / kernel_ms), every repeat in the same process, the variants alternating inside a
repeat:
  * k_score_observed: logistic and linear, c = 4 and c = 8 (the dense walk; the kernel has no set-bit variant);
  * k_ranksum and k_cat_observed, the observed passes of the rank-sum and chi-square tests, on the same matrix and
    ten traits: the yardstick of what a one-gene-per-lane walk over the set bits costs here;
and the host's null fits (score_host) by a host clock.  Before anything is timed the device's sums U and b_0 of every
gene are held to fp64 matrix products of the same rows (1e-9 relative to the sum of the absolute terms).
Reported: median, min and max of each; (isolate, accumulator) additions per second of the dense walk.  Raw lines on
stdout (profiles/score.txt).
    python tools/bench_score.py [repeats] [warmup]"""
import datetime
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from scoary_amd import synth
from scoary_amd.engine import AssociationEngine, score_host

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 2
T = 10

if not torch.cuda.is_available():
    sys.exit("bench_score needs an MI355X: there is nothing to time without one")
genes, _traits, _P, seed = synth.make_config("cfg3", T=1)
G, N = genes.shape
rng = np.random.default_rng(seed + 24)
cov8 = rng.standard_normal((8, N))
cov8[rng.integers(8, size=20), rng.integers(N, size=20)] = np.nan
eta = cov8[:4].T @ rng.standard_normal(4) / 2.0
eta = np.nan_to_num(eta)
binary = (rng.random((T, N)) < 1.0 / (1.0 + np.exp(-(eta[None, :] + rng.standard_normal((T, 1)))))).astype(np.float64)
measured = eta[None, :] + rng.standard_normal((T, N))
for rows in (binary, measured):
    rows[rng.random((T, N)) < 0.01] = np.nan
eng = AssociationEngine(0)
gm = eng.pack_dense(genes)
print("date %s  shape G=%d N=%d T=%d  repeats %d warm-up %d" % (datetime.date.today().isoformat(), G, N, T, REPEATS,
                                                                 WARMUP), flush=True)

plans, host_ms = {}, {}
for kind, values in (("logistic", binary), ("linear", measured)):
    for c in (4, 8):
        t0 = time.perf_counter()
        host = score_host(values, cov8[:c], kind)
        host_ms[kind, c] = (time.perf_counter() - t0) * 1e3
        plans[kind, c] = eng.score_plan_of(host, kind)
        assert plans[kind, c].skipped == [None] * T, plans[kind, c].skipped

# the device's sums against fp64 matrix products of the same rows
dense = torch.from_numpy(genes).to(eng.device).to(torch.float64)
for key, plan in plans.items():
    res = eng.score(gm, plan)
    for name, row in (("U", 0), ("b_0", 1)):
        got = res["U"] if row == 0 else res["b"][:, :, 0]
        want = plan.rows[:, row, :] @ dense.t()
        scale = plan.rows[:, row, :].abs() @ dense.t()
        worst = float(((got - want).abs() / scale.clamp_min(1e-300)).max())
        print("%s c=%d: %s against the matrix product, worst |difference| / sum |terms| = %.3g" % (*key, name, worst),
              flush=True)
        if not worst <= 1e-9:
            sys.exit("the sums disagree: nothing is timed")
    tested = int((res["p"] < 1.0).sum())
    print("%s c=%d: %d of %d (trait, gene) pairs have p < 1" % (*key, tested, T * G), flush=True)
del dense

rank_plan = eng.ranksum_plan(np.where(np.isnan(measured), np.nan, np.round(measured, 1)))
cat_plan = eng.categorical_plan(rng.integers(0, 5, size=(T, N)))


def timed(fn, kernel):
    eng.set_timing(True)
    try:
        fn()
        torch.cuda.synchronize()
        return eng.kernel_ms(kernel)
    finally:
        eng.set_timing(False)


variants = [("k_score_observed %s c=%d" % key, (lambda p=plan: eng.score(gm, p)), "k_score_observed")
            for key, plan in plans.items()]
variants += [("k_ranksum (observed pass)", lambda: eng.ranksum(gm, rank_plan), "k_ranksum"),
             ("k_cat_observed (observed pass, K = 4)", lambda: eng.categorical(gm, cat_plan), "k_cat_observed")]
t = {name: [] for name, _fn, _k in variants}
for i in range(WARMUP + REPEATS):
    for name, fn, kernel in (variants if i % 2 == 0 else variants[::-1]):
        ms = timed(fn, kernel)
        if i >= WARMUP:
            t[name].append(ms)
for name, xs in t.items():
    print("%-44s median %9.3f ms  min %9.3f  max %9.3f  (n=%d)" % (name, statistics.median(xs), min(xs), max(xs),
                                                                   len(xs)), flush=True)
for (kind, c), plan in plans.items():
    ms = statistics.median(t["k_score_observed %s c=%d" % (kind, c)])
    adds = float(G) * T * N * (c + 2)
    print("k_score_observed %s c=%d: %.3g (isolate, accumulator) additions per second (%.3g over the median); "
          "host null fits of %d traits %.1f ms" % (kind, c, adds / (ms * 1e-3), adds, T, host_ms[kind, c]), flush=True)
try:
    import __graft_entry__ as ge
    with open(ge.HIP_RESOURCES) as f:
        res = json.load(f)
    for name, fields in sorted(res.items()):
        if "k_score_observed" in name:
            print("%s: VGPRs %s, SGPRs %s, scratch %s" % (name[:48], fields.get("VGPRs"), fields.get("TotalSGPRs"),
                                                         fields.get("ScratchSize")), flush=True)
except (OSError, ImportError, ValueError):
    print("k_score_observed resources: the build's report was not found", flush=True)
