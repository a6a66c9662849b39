"""The stratified rank-sum permutation step (spec S16) next to the unstratified one (spec S15) at cfg3's geometry
with ten quantitative traits on one MI355X: G = 50 000 genes, N = 2000 isolates, T = 10, P = 10 000 value
permutations, the isolates in 10 and in 1000 strata.

Timed, every repeat in the same process, the three variants alternating inside a repeat (their order reversed in
every other repeat):
  * unstratified: k_ranksum_labels (the generator, B-operand form) and k_permute_ranksum by device events
    (set_timing / kernel_ms), the whole step engine.ranksum_permute by a host clock around a device synchronise;
  * 10 strata and 1000 strata: k_vanelteren_labels and k_permute_ranksum by device events, the whole step
    engine.vanelteren_permute by the host clock; and once, the observed-statistic kernel k_vanelteren.
Before anything is timed the stratified counts are held to an exact fp32 product over the generator's plain rows
(trait 0, the first 512 permutations).  Reported: median, min and max of each and the generators' ratio.  Raw lines
on stdout (profiles/vanelteren.txt).
    python tools/bench_vanelteren.py [repeats] [warmup]"""
import datetime
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from scoary_amd import synth
from scoary_amd.engine import AssociationEngine

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 2
T, CHECK_P = 10, 512

if not torch.cuda.is_available():
    sys.exit("bench_vanelteren needs an MI355X: there is nothing to time without one")
genes, _traits, P, seed = synth.make_config("cfg3", T=1)
G, N = genes.shape
rng = np.random.default_rng(seed + 16)
values = np.round(rng.standard_normal((T, N)) * 2.0, 1)         # measurements with ties
values[rng.random((T, N)) < 0.01] = np.nan
eng = AssociationEngine(0)
gm = eng.pack_dense(genes)
rplan = eng.ranksum_plan(values)
rd = eng.ranksum(gm, rplan)["d"]
plans = {}
for S in (10, 1000):
    st = rng.integers(0, S, N)
    st[:S] = np.arange(S)                                       # every stratum in use
    plan = eng.vanelteren_plan(values, st)
    plans[S] = (plan, eng.vanelteren(gm, plan))
print("date %s  shape G=%d N=%d T=%d P=%d  repeats %d warm-up %d" % (
    datetime.date.today().isoformat(), G, N, T, P, REPEATS, WARMUP), flush=True)


def sync_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def timed(fn, label_kernel):
    eng.set_timing(True)
    try:
        r, ms = sync_ms(fn)
        return r, dict(step=ms, labels=eng.kernel_ms(label_kernel), permute=eng.kernel_ms("k_permute_ranksum"))
    finally:
        eng.set_timing(False)


variants = {"unstratified": (lambda: eng.ranksum_permute(gm, rplan, rd, P, seed), "k_ranksum_labels")}
for S, (plan, obs) in plans.items():
    variants["%d strata" % S] = (lambda plan=plan, obs=obs: eng.vanelteren_permute(gm, plan, obs["d"], P, seed),
                                 "k_vanelteren_labels")

dense = torch.from_numpy(genes).to(eng.device).to(torch.float64)
for S, (plan, obs) in plans.items():
    # |a| <= 16319 and at most N = 2000 terms: every partial sum is an integer below 2^25 -- past fp32's 2^24, so
    # the product runs in fp64
    rows = eng.vanelteren_values(plan, 0, CHECK_P, seed)[0].to(torch.float64).t().contiguous()
    want = ((dense @ rows).abs_() >= obs["d"][0].abs().to(torch.float64)[:, None]).sum(dim=1)
    got = eng.vanelteren_permute(gm, plan, obs["d"], CHECK_P, seed)[0].to(torch.int64)
    bad = int((got != want).sum())
    print("%4d strata: r over %d permutations against the exact fp64 product: %d of %d genes differ; %d genes "
          "testable in trait 0" % (S, CHECK_P, bad, G, int((obs["var"][0] > 0).sum())), flush=True)
    if bad:
        sys.exit("the counts disagree: nothing is timed")
    eng.set_timing(True)
    eng.vanelteren(gm, plan)
    torch.cuda.synchronize()
    print("%4d strata: k_vanelteren (observed statistic, T = %d) %.3f ms, k_cmh_segments %.3f ms" % (
        S, T, eng.kernel_ms("k_vanelteren"), eng.kernel_ms("k_cmh_segments")), flush=True)
    eng.set_timing(False)
del dense

t = {name: dict(step=[], labels=[], permute=[]) for name in variants}
for i in range(WARMUP + REPEATS):
    order = list(variants)
    for name in (order if i % 2 == 0 else order[::-1]):
        fn, kernel = variants[name]
        _r, got = timed(fn, kernel)
        if i >= WARMUP:
            for k, v in got.items():
                t[name][k].append(v)


def line(name, xs):
    print("%-52s median %9.3f ms  min %9.3f  max %9.3f  (n=%d)" % (name, statistics.median(xs), min(xs), max(xs),
                                                                   len(xs)), flush=True)


for name, (fn, kernel) in variants.items():
    line("%s: %s (generator, B form)" % (name, kernel), t[name]["labels"])
    line("%s: k_permute_ranksum" % name, t[name]["permute"])
    line("%s: whole step (host clock)" % name, t[name]["step"])
base = statistics.median(t["unstratified"]["labels"])
for name in list(variants)[1:]:
    print("%s: k_vanelteren_labels / k_ranksum_labels = %.3f; whole step / unstratified step = %.3f" % (
        name, statistics.median(t[name]["labels"]) / base,
        statistics.median(t[name]["step"]) / statistics.median(t["unstratified"]["step"])), flush=True)
try:            # clocks and power: read, never set
    smi = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=30)
    rows = [ln.strip() for ln in smi.stdout.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "Power" in ln)]
    print("telemetry after the run (rocm-smi, GPU 0): " + ("; ".join(rows) if rows else "not read"), flush=True)
except (OSError, subprocess.SubprocessError):
    print("telemetry: clocks and power not read", flush=True)
