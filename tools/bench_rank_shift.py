"""The Hodges-Lehmann shift stage (spec S19, k_rank_shift) next to the permutation run of the stage it belongs to, at
cfg3's geometry with ten quantitative traits on one MI355X: G = 50 000 genes, N = 2000 isolates, T = 10.

Timed, every repeat in the same process, the variants alternating inside a repeat (their order reversed in every
other repeat):
  * k_rank_shift by device events (set_timing / kernel_ms) through its raw entry point, on four inputs: values all
    distinct or MIC-like (sixteen two-fold dilutions: heavy ties), gene frequencies U-shaped (cfg3's) or all near 50 %;
  * the whole stage by a host clock around a device synchronise: engine.ranksum_shift (var, the kernel) on the first
    input;
  * the yardstick, on code the stage does not touch: engine.ranksum_permute with P = 10 000 on cfg3's genes, the
    permutation run of --quantitative --permute 10000.
Before anything is timed a sample of genes of every input is held to numpy: the shift to numpy.median of the
differences bit for bit, the limits to the sorted differences at the device's ca.  That check's own time on its
sample is printed and labelled as such; it is no comparison of speed.  Reported: median, min and max of each and the
ratio shift stage / permutation run (the bar: at most 1).  Raw lines on stdout (profiles/rank_shift.txt).
    python tools/bench_rank_shift.py [repeats] [warmup]"""
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
T, LEVEL, SAMPLE = 10, 0.95, 24

if not torch.cuda.is_available():
    sys.exit("bench_rank_shift needs an MI355X: there is nothing to time without one")
genes_u, _traits, P, seed = synth.make_config("cfg3", T=1)
G, N = genes_u.shape
rng = np.random.default_rng(seed + 19)
genes_half = (rng.random((G, N)) < rng.uniform(0.45, 0.55, (G, 1))).astype(np.uint8)
distinct = rng.standard_normal((T, N)) * 2.0
mic = np.exp2(rng.integers(-8, 8, (T, N)).astype(np.float64))
for v in (distinct, mic):
    v[rng.random((T, N)) < 0.01] = np.nan
eng = AssociationEngine(0)
print("date %s  shape G=%d N=%d T=%d P=%d  level %.2f  repeats %d warm-up %d" % (
    datetime.date.today().isoformat(), G, N, T, P, LEVEL, REPEATS, WARMUP), flush=True)


def sync_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def kernel(fn, name):
    eng.set_timing(True)
    try:
        fn()
        torch.cuda.synchronize()
        return eng.kernel_ms(name)
    finally:
        eng.set_timing(False)


inputs = {}
for gname, dense in (("U-shaped", genes_u), ("near 50 %", genes_half)):
    gm = eng.pack_dense(dense)
    for vname, values in (("distinct", distinct), ("MIC-like", mic)):
        plan = eng.ranksum_plan(values)
        res = eng.ranksum(gm, plan)
        inputs["%s values, %s genes" % (vname, gname)] = (gm, plan, res, dense, values)

# -- the checks: nothing is timed that computes something else
for name, (gm, plan, res, dense, values) in inputs.items():
    out = {k: v.cpu().numpy() for k, v in eng.ranksum_shift(gm, plan, res, level=LEVEL).items()}
    m = res["m"].cpu().numpy()
    bad, spent, minority = 0, 0.0, np.minimum(m, plan.n[:, None] - m)
    for g in rng.integers(0, G, SAMPLE):
        t = int(rng.integers(0, T))
        valid = ~np.isnan(values[t])
        t0 = time.perf_counter()
        d = np.sort(np.subtract.outer(values[t][valid & (dense[g] == 1)], values[t][valid & (dense[g] == 0)]).ravel())
        spent += time.perf_counter() - t0
        ca = int(out["ca"][t, g])
        if d.size == 0 or not np.isfinite(out["upper"][t, g]):
            continue
        want = (np.median(d) + 0.0, d[ca - 1] + 0.0, d[d.size - ca] + 0.0)
        got = (out["shift"][t, g], out["lower"][t, g], out["upper"][t, g])
        bad += np.asarray(want).tobytes() != np.asarray(got).tobytes()
    print("%-38s %d of %d sampled genes differ from numpy (numpy's sort of those %d genes' differences: %.1f ms -- "
          "the check's own time, not a comparison); mean smaller side %.0f isolates"
          % (name, bad, SAMPLE, SAMPLE, spent * 1e3, float(minority.mean())), flush=True)
    if bad:
        sys.exit("the shift stage disagrees with numpy: nothing is timed")

gm0, plan0, res0 = next(iter(inputs.values()))[:3]


def shift_pass(gm, plan, res):
    return lambda: eng.ranksum_shift(gm, plan, res, level=LEVEL)


variants = {"k_rank_shift, " + name: (lambda gm=gm, plan=plan, res=res: kernel(shift_pass(gm, plan, res), "k_rank_shift"))
            for name, (gm, plan, res, _d, _v) in inputs.items()}
variants["stage with the flag (ranksum_shift), first input"] = lambda: sync_ms(shift_pass(gm0, plan0, res0))[1]
variants["permutation run (ranksum_permute, P = %d)" % P] = lambda: sync_ms(
    lambda: eng.ranksum_permute(gm0, plan0, res0["d"], P, seed))[1]
t = {name: [] for name in variants}
for i in range(WARMUP + REPEATS):
    order = list(variants)
    for name in (order if i % 2 == 0 else order[::-1]):
        ms = variants[name]()
        if i >= WARMUP:
            t[name].append(ms)
    print("round %d of %d done" % (i + 1, WARMUP + REPEATS), flush=True)

for name, xs in t.items():
    print("%-62s median %9.3f ms  min %9.3f  max %9.3f  (n=%d)" % (name, statistics.median(xs), min(xs), max(xs),
                                                                   len(xs)), flush=True)
med = {name: statistics.median(xs) for name, xs in t.items()}
perm = med["permutation run (ranksum_permute, P = %d)" % P]
for name in variants:
    if name.startswith("k_rank_shift") or name.startswith("stage"):
        print("%-62s / permutation run = %.3f (the bar: at most 1)" % (name, med[name] / perm), flush=True)
try:            # clocks and power: read, never set
    smi = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=30)
    lines = [ln.strip() for ln in smi.stdout.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "Power" in ln)]
    print("telemetry after the run (rocm-smi, GPU 0): " + ("; ".join(lines) if lines else "not read"), flush=True)
except (OSError, subprocess.SubprocessError):
    print("telemetry: clocks and power not read", flush=True)
