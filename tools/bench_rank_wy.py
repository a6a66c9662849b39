"""The fused Westfall-Young pass over the rank statistics (spec S17) next to the count pass it extends, at cfg3's
geometry with ten quantitative traits on one MI355X: G = 50 000 genes, N = 2000 isolates, T = 10, P = 10 000 value
permutations.

Timed, every repeat in the same process, the variants alternating inside a repeat (their order reversed in every
other repeat):
  * k_permute_ranksum and k_rank_maxt by device events (set_timing / kernel_ms), each launched through its raw
    entry point over ONE B operand, generated once; maxs is zeroed before every launch of k_rank_maxt, so that its
    combine meets what the first batch of a run meets and not a row that already holds the maxima;
  * the whole permutation step by a host clock around a device synchronise: engine.ranksum_permute (the step without
    --quantitative-fwer) and engine.ranksum_westfall_young (the step with it: var, iv and s_obs, the fused pass, the
    sort and the search).
Before anything is timed the fused pass is held to the count pass (d_r, all of it) and to an exact fp64 product over
the generator's plain rows (maxs of trait 0, the first 512 permutations, bit for bit).  Reported: median, min and max
of each, and the ratio the bar is set on: k_rank_maxt must take less than twice k_permute_ranksum's time, the cost
of the count pass plus a second product of the same size for the maxima.  Raw lines on stdout (profiles/rank_wy.txt).
    python tools/bench_rank_wy.py [repeats] [warmup]"""
import ctypes
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
    sys.exit("bench_rank_wy needs an MI355X: there is nothing to time without one")
genes, _traits, P, seed = synth.make_config("cfg3", T=1)
G, N = genes.shape
rng = np.random.default_rng(seed + 16)
values = np.round(rng.standard_normal((T, N)) * 2.0, 1)         # measurements with ties (bench_vanelteren's)
values[rng.random((T, N)) < 0.01] = np.nan
eng = AssociationEngine(0)
gm = eng.pack_dense(genes)
plan = eng.ranksum_plan(values)
res = eng.ranksum(gm, plan)
iv, sobs = eng.rank_wy_prepare(eng.ranksum_var(plan, res["m"]), res["d"], 1)
print("date %s  shape G=%d N=%d T=%d P=%d  repeats %d warm-up %d" % (
    datetime.date.today().isoformat(), G, N, T, P, REPEATS, WARMUP), flush=True)

bfrag = torch.empty((int(eng.lib.scoary_ranksum_bfrag_bytes(N, P, T)),), dtype=torch.uint8, device=eng.device)
eng._check(eng.lib.scoary_ranksum_perm_generate_bfrag(
    eng.h, eng._ptr(plan.rc), eng._ptr(plan.valid), T, N, P, 0, 0, ctypes.c_uint64(seed), eng._ptr(bfrag),
    eng._stream()), "scoary_ranksum_perm_generate_bfrag")
r_count = torch.zeros((T, G), dtype=torch.int32, device=eng.device)
r_maxt = torch.zeros((T, G), dtype=torch.int32, device=eng.device)
maxs = torch.zeros((T, P), dtype=torch.float64, device=eng.device)


def count_pass():
    r_count.zero_()
    eng._check(eng.lib.scoary_permute_ranksum(eng.h, eng._ptr(gm.tiled), eng._ptr(bfrag), eng._ptr(res["d"]), G, T, N,
                                              P, eng._ptr(r_count), eng._stream()), "scoary_permute_ranksum")


def maxt_pass():
    r_maxt.zero_()
    maxs.zero_()
    eng._check(eng.lib.scoary_permute_rank_wy(
        eng.h, eng._ptr(gm.tiled), eng._ptr(bfrag), eng._ptr(res["d"]), eng._ptr(iv), 1, G, T, N, P, eng._ptr(r_maxt),
        eng._ptr(maxs), P, eng._stream()), "scoary_permute_rank_wy")


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


# -- the checks: nothing is timed that computes something else
count_pass()
maxt_pass()
torch.cuda.synchronize()
bad = int((r_count != r_maxt).sum())
print("d_r of k_rank_maxt against k_permute_ranksum: %d of %d cells differ" % (bad, T * G), flush=True)
dense = torch.from_numpy(genes).to(eng.device).to(torch.float64)
# |Rc| < 2000 and at most N = 2000 terms: every partial sum is an integer below 2^22, exact in fp64; E, E * E and
# (E * E) * iv are the spec's own operations, each rounded once (no fused multiply-add between separate torch calls)
rows = eng.ranksum_values(plan, 0, CHECK_P, seed)[0].to(torch.float64).t().contiguous()
e = ((dense @ rows).abs_() - 1.0).clamp_(min=0.0)
want = ((e * e) * iv[0][:, None]).max(dim=0).values
bad_m = int((want.view(torch.int64) != maxs[0, :CHECK_P].view(torch.int64)).sum())
print("maxs of trait 0 over %d permutations against the exact fp64 product: %d differ; %d genes testable in trait 0"
      % (CHECK_P, bad_m, int((iv[0] > 0).sum())), flush=True)
del dense, rows, e, want
if bad or bad_m:
    sys.exit("the fused pass disagrees: nothing is timed")
r_step, rf_step, mx_step = eng.ranksum_westfall_young(gm, plan, res, P, seed)
if not (torch.equal(r_step, r_count) and torch.equal(mx_step, maxs)):
    sys.exit("the engine's step disagrees with the raw entry points: nothing is timed")
print("r_fwer of trait 0: %d genes at 0, %d below 5 %% of P, r_fwer >= r_q in %d of %d cells" % (
    int((rf_step[0] == 0).sum()), int((rf_step[0] < P // 20).sum()), int((rf_step >= r_step).sum()), T * G), flush=True)

variants = {
    "k_permute_ranksum": lambda: kernel(count_pass, "k_permute_ranksum"),
    "k_rank_maxt": lambda: kernel(maxt_pass, "k_rank_maxt"),
    "step without the flag (ranksum_permute)": lambda: sync_ms(
        lambda: eng.ranksum_permute(gm, plan, res["d"], P, seed))[1],
    "step with the flag (ranksum_westfall_young)": lambda: sync_ms(
        lambda: eng.ranksum_westfall_young(gm, plan, res, P, seed))[1],
}
t = {name: [] for name in variants}
for i in range(WARMUP + REPEATS):
    order = list(variants)
    for name in (order if i % 2 == 0 else order[::-1]):
        ms = variants[name]()
        if i >= WARMUP:
            t[name].append(ms)

for name, xs in t.items():
    print("%-46s median %9.3f ms  min %9.3f  max %9.3f  (n=%d)" % (name, statistics.median(xs), min(xs), max(xs),
                                                                   len(xs)), flush=True)
med = {name: statistics.median(xs) for name, xs in t.items()}
ratio = med["k_rank_maxt"] / med["k_permute_ranksum"]
print("k_rank_maxt / k_permute_ranksum = %.3f (the bar: below 2); step with / without the flag = %.3f" % (
    ratio, med["step with the flag (ranksum_westfall_young)"] / med["step without the flag (ranksum_permute)"]),
    flush=True)
try:            # clocks and power: read, never set
    smi = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=30)
    lines = [ln.strip() for ln in smi.stdout.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "Power" in ln)]
    print("telemetry after the run (rocm-smi, GPU 0): " + ("; ".join(lines) if lines else "not read"), flush=True)
except (OSError, subprocess.SubprocessError):
    print("telemetry: clocks and power not read", flush=True)
