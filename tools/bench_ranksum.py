"""The rank-sum permutation step (spec S15) at cfg3's geometry with one quantitative trait on one MI355X:
G = 50 000 genes, N = 2000 isolates, P = 10 000 value permutations.

Timed, every repeat in the same process, the variants alternating inside a repeat:
  * k_ranksum_labels (the generator, B-operand form) and k_permute_ranksum, each by device events (set_timing /
    kernel_ms), and the whole step engine.ranksum_permute by a host clock around a device synchronise;
  * the yardstick, the library formulation of the same count on the same data: the gene matrix unpacked to 0/1
    (bf16 operands with an fp32 result, where the digits and the accumulation are exact at this size;
    torch._int_mm on int8 as well where this torch build runs it) times the two digit planes of the generator's
    plain rows, in permutation batches, D = 128 D_hi + D_lo, |D| >= |D_obs| counted -- both held to an exact fp32
    product before anything is timed;
  * the plain Fisher permutation step (associate, list path) of one binary trait on the same matrix.
Reported: median, min and max of each, the int8 multiply-adds per second of k_permute_ranksum (G N P for each of the
two digit planes), its ratio to the yardstick with the yardstick's own spread, and the ratio to the Fisher step.
Raw lines on stdout (profiles/ranksum.txt).
    python tools/bench_ranksum.py [repeats] [warmup]"""
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
from scoary_amd.engine import AssociationEngine, pack_bits_rows

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 2
YARD_BATCH = 2048                      # permutations per yardstick batch: a 50 000 x 2048 fp32 product is 400 MB

if not torch.cuda.is_available():
    sys.exit("bench_ranksum needs an MI355X: there is nothing to time without one")
genes, traits, P, seed = synth.make_config("cfg3", T=1)
G, N = genes.shape
rng = np.random.default_rng(seed + 15)
values = np.round(rng.standard_normal((1, N)) * 2.0, 1)         # a measurement with ties
values[0, rng.random(N) < 0.01] = np.nan
eng = AssociationEngine(0)
gm = eng.pack_dense(genes)
plan = eng.ranksum_plan(values)
obs = eng.ranksum(gm, plan)
d_obs = obs["d"]
print("date %s  shape G=%d N=%d T=1 P=%d  n=%d tie groups=%d  repeats %d warm-up %d" % (
    datetime.date.today().isoformat(), G, N, P, int(plan.n[0]), int(plan.tie_groups[0]), REPEATS, WARMUP), flush=True)


def sync_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def ours():
    eng.set_timing(True)
    try:
        r, ms = sync_ms(lambda: eng.ranksum_permute(gm, plan, d_obs, P, seed))
        return r, ms, eng.kernel_ms("k_ranksum_labels"), eng.kernel_ms("k_permute_ranksum")
    finally:
        eng.set_timing(False)


dense = torch.from_numpy(genes).to(eng.device)
a_bf16 = dense.to(torch.bfloat16)
a_i8 = dense.to(torch.int8)
thr = d_obs[0].abs().to(torch.int64)


def digit_planes(rows):
    """int16 [p, N] -> (hi, lo) int16 [N, p], Rc = 128 hi + lo with lo in [-64, 63]."""
    rc = rows.to(torch.int32)
    lo = ((rc + 64) & 127) - 64
    return ((rc - lo) >> 7).t().contiguous(), lo.t().contiguous()


def yardstick(kind):
    """(r, ms of products + compare + count, ms of the whole step with the generator and the digit split)."""
    r = torch.zeros(G, dtype=torch.int64, device=eng.device)
    torch.cuda.synchronize()
    t_all = time.perf_counter()
    gemm_ms = 0.0
    for base in range(0, P, YARD_BATCH):
        pb = min(YARD_BATCH, P - base)
        hi, lo = digit_planes(eng.ranksum_values(plan, base, pb, seed)[0])
        if kind == "bf16":
            hi, lo = hi.to(torch.bfloat16), lo.to(torch.bfloat16)
        else:
            hi, lo = hi.to(torch.int8), lo.to(torch.int8)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "bf16":
            # (bf16 operands, fp32 result: a bf16 result would round the sums)
            d = (torch.mm(a_bf16, hi, out_dtype=torch.float32) * 128.0
                 + torch.mm(a_bf16, lo, out_dtype=torch.float32)).abs_()
            r += (d >= thr[:, None].float()).sum(dim=1)
        else:
            d = (torch._int_mm(a_i8, hi) * 128 + torch._int_mm(a_i8, lo)).abs_()
            r += (d >= thr[:, None]).sum(dim=1)
        torch.cuda.synchronize()
        gemm_ms += (time.perf_counter() - t0) * 1e3
    return r, gemm_ms, (time.perf_counter() - t_all) * 1e3


def exact_reference():
    """r_q by an fp32 product of the 0/1 matrix with the undivided ranks: every partial sum is an integer below
    2^24, so it is exact whatever the order of the sum (fp32 GEMM has no reduced-precision path on this chip)."""
    a_f32 = dense.to(torch.float32)
    r = torch.zeros(G, dtype=torch.int64, device=eng.device)
    for base in range(0, P, YARD_BATCH):
        pb = min(YARD_BATCH, P - base)
        rc = eng.ranksum_values(plan, base, pb, seed)[0].to(torch.float32).t().contiguous()
        r += (torch.matmul(a_f32, rc).abs_() >= thr[:, None].float()).sum(dim=1)
    return r


r_ref = exact_reference()
r_ours = ours()[0][0].to(torch.int64)
print("k_permute_ranksum against the exact fp32 product: %d of %d genes differ" % (int((r_ours != r_ref).sum()), G),
      flush=True)
kinds = []
for kind in ("bf16", "int8"):
    try:
        bad = int((yardstick(kind)[0] != r_ref).sum())
    except (RuntimeError, TypeError, NotImplementedError) as e:
        print("yardstick %s: not run by this torch build (%s)" % (kind, str(e).splitlines()[0][:160]), flush=True)
        continue
    print("yardstick %s against the exact fp32 product: %d of %d genes differ" % (kind, bad, G), flush=True)
    if bad == 0:
        kinds.append(kind)
if int((r_ours != r_ref).sum()) or not kinds:
    sys.exit("the counts disagree: nothing is timed")
print("r_q < P on %d of the %d genes" % (int((r_ours < P).sum()), G), flush=True)

# the plain Fisher permutation step of one binary trait on the same matrix
trv = eng.vecrows(pack_bits_rows((traits == 1).astype(np.uint8)), N)
mkv = eng.vecrows(pack_bits_rows((traits != 2).astype(np.uint8)), N)
eng.build_lists(gm)


def fisher_step():
    return sync_ms(lambda: eng.associate(gm, trv, mkv, permutations=P, seed=seed, use_lists=True))[1]


t = {k: [] for k in ["step", "labels", "permute", "fisher"] + ["yard_" + k for k in kinds]
     + ["yard_step_" + k for k in kinds]}
for i in range(WARMUP + REPEATS):
    keep = i >= WARMUP
    order = ["ours"] + kinds + ["fisher"]
    for which in (order if i % 2 == 0 else order[::-1]):
        if which == "ours":
            _r, ms, lab, perm = ours()
            got = dict(step=ms, labels=lab, permute=perm)
        elif which == "fisher":
            got = dict(fisher=fisher_step())
        else:
            _r, gemm, whole = yardstick(which)
            got = {"yard_" + which: gemm, "yard_step_" + which: whole}
        if keep:
            for k, v in got.items():
                t[k].append(v)


def line(name, xs):
    print("%-44s median %9.3f ms  min %9.3f  max %9.3f  (n=%d)" % (name, statistics.median(xs), min(xs), max(xs),
                                                                   len(xs)), flush=True)


line("k_ranksum_labels (generator, B form)", t["labels"])
line("k_permute_ranksum", t["permute"])
line("ranksum_permute (whole step, host clock)", t["step"])
for k in kinds:
    line("yardstick %s: products + compare + count" % k, t["yard_" + k])
    line("yardstick %s: whole step with generator" % k, t["yard_step_" + k])
line("Fisher permutation step (associate, lists)", t["fisher"])
perm = statistics.median(t["permute"])
print("k_permute_ranksum: %.3g int8 multiply-adds per second (2 G N P = %.3g over the median)" % (
    2.0 * G * N * P / (perm * 1e-3), 2.0 * G * N * P), flush=True)
for k in kinds:
    y = t["yard_" + k]
    spread = max(y) - min(y)
    print("k_permute_ranksum / yardstick %s = %.3f; the yardstick's run-to-run spread is %.3f ms (%.1f %% of its "
          "median): the kernel is %s the yardstick plus twice that spread" % (
              k, perm / statistics.median(y), spread, 100.0 * spread / statistics.median(y),
              "within" if perm <= statistics.median(y) + 2.0 * spread else "slower than"), flush=True)
print("ranksum_permute / Fisher permutation step = %.3f" % (statistics.median(t["step"]) /
                                                            statistics.median(t["fisher"])), flush=True)
try:            # clocks and power: read, never set
    smi = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=30)
    rows = [ln.strip() for ln in smi.stdout.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "Power" in ln)]
    print("telemetry after the run (rocm-smi, GPU 0): " + ("; ".join(rows) if rows else "not read"), flush=True)
except (OSError, subprocess.SubprocessError):
    print("telemetry: clocks and power not read", flush=True)
