"""The step-down maxT passes over the rank statistics (spec S18) next to the single-step pass and the count pass they
restate, at cfg3's geometry with ten quantitative traits on one MI355X: G = 50 000 genes, N = 2000 isolates (or the
first N of them), T = 10, P = 10 000 value permutations.

Timed, every repeat in the same process, the variants alternating inside a repeat (their order reversed in every
other repeat):
  * k_permute_ranksum and k_rank_maxt (the yardsticks), k_rank_sd_max, k_rank_sd_suffix and k_rank_sd_count (one call
    of scoary_permute_rank_stepdown) and k_rank_sd_gather by device events (set_timing / kernel_ms), each launched
    through its raw entry point over ONE B operand, generated once;
  * the whole permutation step by a host clock around a device synchronise: engine.ranksum_permute (no family-wise
    flag), engine.ranksum_westfall_young (--quantitative-fwer) and engine.ranksum_stepdown
    (--quantitative-fwer-stepdown: the sort, the gather, the three launches, the tail and the single-step search).
Before anything is timed the step-down passes are held to the other two kernels (r by rank position against
k_permute_ranksum's d_r, maxs against k_rank_maxt's, all of both) and to an exact fp64 product over the generator's
plain rows (c of trait 0 over the first 512 permutations, every rank).  Reported: median, min and max of each, and the
two passes together against k_rank_maxt: the product is formed twice, so about 2 x is what the design predicts.
Raw lines on stdout (profiles/rank_stepdown.txt).
    python tools/bench_rank_stepdown.py [repeats] [warmup] [isolates]"""
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
    sys.exit("bench_rank_stepdown needs an MI355X: there is nothing to time without one")
genes, _traits, P, seed = synth.make_config("cfg3", T=1)
if len(sys.argv) > 3:
    genes = np.ascontiguousarray(genes[:, :int(sys.argv[3])])
G, N = genes.shape
rng = np.random.default_rng(seed + 16)
values = np.round(rng.standard_normal((T, N)) * 2.0, 1)         # measurements with ties (bench_rank_wy's)
values[rng.random((T, N)) < 0.01] = np.nan
eng = AssociationEngine(0)
gm = eng.pack_dense(genes)
plan = eng.ranksum_plan(values)
res = eng.ranksum(gm, plan)
iv, sobs = eng.rank_wy_prepare(eng.ranksum_var(plan, res["m"]), res["d"], 1)
order32, ss = eng.rank_stepdown_order(sobs)
print("date %s  shape G=%d N=%d T=%d P=%d  repeats %d warm-up %d" % (
    datetime.date.today().isoformat(), G, N, T, P, REPEATS, WARMUP), flush=True)

bfrag = torch.empty((int(eng.lib.scoary_ranksum_bfrag_bytes(N, P, T)),), dtype=torch.uint8, device=eng.device)
eng._check(eng.lib.scoary_ranksum_perm_generate_bfrag(
    eng.h, eng._ptr(plan.rc), eng._ptr(plan.valid), T, N, P, 0, 0, ctypes.c_uint64(seed), eng._ptr(bfrag),
    eng._stream()), "scoary_ranksum_perm_generate_bfrag")
scratch = eng.rank_stepdown_gather(gm, order32, sobs, iv, res["d"], N, P)
print("scratch %.1f MB (gmax %.1f MB), B operand %.1f MB" % (
    scratch.numel() / 1e6, 8e-6 * T * (eng.padded_genes(G) // 64) * (-(-P // 64) * 64), bfrag.numel() / 1e6), flush=True)
r_count = torch.zeros((T, G), dtype=torch.int32, device=eng.device)
r_maxt = torch.zeros((T, G), dtype=torch.int32, device=eng.device)
r_rank = torch.zeros((T, G), dtype=torch.int32, device=eng.device)
c_rank = torch.zeros((T, G), dtype=torch.int32, device=eng.device)
maxs = torch.zeros((T, P), dtype=torch.float64, device=eng.device)
maxs_sd = torch.zeros((T, P), dtype=torch.float64, device=eng.device)


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


def sd_passes():
    r_rank.zero_()
    c_rank.zero_()
    eng.permute_rank_stepdown(scratch, bfrag, 1, G, T, N, P, 0, r_rank, c_rank, maxs_sd)


def gather_pass():
    eng._check(eng.lib.scoary_rank_stepdown_gather(
        eng.h, eng._ptr(gm.tiled), eng._ptr(order32), eng._ptr(sobs), eng._ptr(iv), eng._ptr(res["d"]), G, T, N,
        eng._ptr(scratch), eng._stream()), "scoary_rank_stepdown_gather")


def sync_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def kernel(fn, *names):
    eng.set_timing(True)
    try:
        fn()
        torch.cuda.synchronize()
        return [eng.kernel_ms(name) for name in names]
    finally:
        eng.set_timing(False)


# -- the checks: nothing is timed that computes something else
count_pass()
maxt_pass()
sd_passes()
torch.cuda.synchronize()
bad_r = int((r_rank != r_count.gather(1, order32.to(torch.int64))).sum())
bad_m = int((maxs_sd.view(torch.int64) != maxs.view(torch.int64)).sum())
print("r by rank against k_permute_ranksum: %d of %d cells differ; maxs against k_rank_maxt: %d of %d differ" % (
    bad_r, T * G, bad_m, T * P), flush=True)
# c of trait 0 over the first CHECK_P permutations, from an exact fp64 product (bench_rank_wy's argument: every
# partial sum is an integer below 2^22; E, E * E and (E * E) * iv are the spec's operations, each rounded once)
c_chk = torch.zeros((T, G), dtype=torch.int32, device=eng.device)
eng.permute_rank_stepdown(scratch, bfrag, 1, G, T, N, CHECK_P, 0, torch.zeros_like(c_chk), c_chk, torch.zeros_like(maxs))
dense = torch.from_numpy(genes).to(eng.device).to(torch.float64)[order32[0].to(torch.int64)]
rows = eng.ranksum_values(plan, 0, CHECK_P, seed)[0].to(torch.float64).t().contiguous()
e = ((dense @ rows).abs_() - 1.0).clamp_(min=0.0)
s = (e * e) * iv[0][order32[0].to(torch.int64)][:, None]
u = torch.flip(torch.cummax(torch.flip(s, dims=(0,)), dim=0).values, dims=(0,))
want_c = (u >= ss[0][:, None]).sum(dim=1).to(torch.int32)
bad_c = int((want_c != c_chk[0]).sum())
print("c of trait 0 over %d permutations against the exact fp64 product: %d of %d ranks differ" % (CHECK_P, bad_c, G),
      flush=True)
del dense, rows, e, s, u, want_c
if bad_r or bad_m or bad_c:
    sys.exit("the step-down passes disagree: nothing is timed")
r_step, rf_step, rsd_step, mx_step = eng.ranksum_stepdown(gm, plan, res, P, seed)
if not (torch.equal(r_step, r_count) and torch.equal(mx_step, maxs)):
    sys.exit("the engine's step disagrees with the raw entry points: nothing is timed")
print("r_q <= r_sd in %d, r_sd <= r_fwer in %d, r_sd < r_fwer in %d of %d cells" % (
    int((r_step <= rsd_step).sum()), int((rsd_step <= rf_step).sum()), int((rsd_step < rf_step).sum()), T * G),
    flush=True)
del r_step, rf_step, rsd_step, mx_step

SD = ("k_rank_sd_max", "k_rank_sd_suffix", "k_rank_sd_count")
variants = {
    "k_permute_ranksum": lambda: kernel(count_pass, "k_permute_ranksum"),
    "k_rank_maxt": lambda: kernel(maxt_pass, "k_rank_maxt"),
    SD: lambda: kernel(sd_passes, *SD),
    "k_rank_sd_gather": lambda: kernel(gather_pass, "k_rank_sd_gather"),
    "step, no family-wise flag (ranksum_permute)": lambda: [sync_ms(
        lambda: eng.ranksum_permute(gm, plan, res["d"], P, seed))[1]],
    "step, --quantitative-fwer (ranksum_westfall_young)": lambda: [sync_ms(
        lambda: eng.ranksum_westfall_young(gm, plan, res, P, seed))[1]],
    "step, --quantitative-fwer-stepdown (ranksum_stepdown)": lambda: [sync_ms(
        lambda: eng.ranksum_stepdown(gm, plan, res, P, seed))[1]],
}
t = {}
for i in range(WARMUP + REPEATS):
    order = list(variants)
    for key in (order if i % 2 == 0 else order[::-1]):
        ms = variants[key]()
        if i >= WARMUP:
            for name, x in zip(key if isinstance(key, tuple) else (key,), ms):
                t.setdefault(name, []).append(x)

med = {name: statistics.median(xs) for name, xs in t.items()}
for name in ["k_permute_ranksum", "k_rank_maxt", *SD, "k_rank_sd_gather"] + [k for k in variants if str(k).startswith("step")]:
    xs = t[name]
    print("%-54s median %9.3f ms  min %9.3f  max %9.3f  (n=%d)" % (name, med[name], min(xs), max(xs), len(xs)),
          flush=True)
both = med["k_rank_sd_max"] + med["k_rank_sd_count"]
print("k_rank_sd_max / k_rank_maxt = %.3f; k_rank_sd_count / k_rank_maxt = %.3f; both passes / k_rank_maxt = %.3f "
      "(the design predicts about 2); with the suffix walk %.3f" % (
          med["k_rank_sd_max"] / med["k_rank_maxt"], med["k_rank_sd_count"] / med["k_rank_maxt"],
          both / med["k_rank_maxt"], (both + med["k_rank_sd_suffix"]) / med["k_rank_maxt"]), flush=True)
print("step with --quantitative-fwer-stepdown / with --quantitative-fwer = %.3f; / without either = %.3f" % (
    med["step, --quantitative-fwer-stepdown (ranksum_stepdown)"] / med["step, --quantitative-fwer (ranksum_westfall_young)"],
    med["step, --quantitative-fwer-stepdown (ranksum_stepdown)"] / med["step, no family-wise flag (ranksum_permute)"]),
    flush=True)
try:            # clocks and power: read, never set
    smi = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=30)
    lines = [ln.strip() for ln in smi.stdout.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "Power" in ln)]
    print("telemetry after the run (rocm-smi, GPU 0): " + ("; ".join(lines) if lines else "not read"), flush=True)
except (OSError, subprocess.SubprocessError):
    print("telemetry: clocks and power not read", flush=True)
