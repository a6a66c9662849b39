"""The stratified categorical permutation step (spec S21) at cfg3's geometry with one trait of K = 4 classes on one
MI355X: G = 50 000 genes (Roary-like frequencies from synth), N = 2000 isolates, P = 10 000 label permutations, over
10 strata and over 1000 strata.

Timed, every repeat in the same process, the variants alternating inside a repeat:
  * k_gcmh_permute against k_cat_permute (spec S20's kernel on the same genes and codes), and the two generators
    (k_vanelteren_labels, k_ranksum_labels), each by device events (set_timing / kernel_ms);
  * the stratified step engine.gcmh_permute against the S20 step engine.categorical_permute, by a host clock around a
    device synchronise; and k_gcmh_observed with its segment table once per strata count.
Before anything is timed the counts of k_gcmh_permute are held to the same rule in torch on the generator's rows (a_k
by fp32 matrix products, exact; the form's quadratic in fp64, one elementwise operation after the other, so every
operation is rounded on its own as in the kernel).
Reported: median, min and max of each and the two ratios with the parent's run-to-run spread -- reported, not gated.
Raw lines on stdout (profiles/gcmh.txt).
    python tools/bench_gcmh.py [repeats] [warmup]
    python tools/bench_gcmh.py shapes         the two permutation kernels alone on random genes at N = 1024 and 1280
                                              (where k_cat_permute fits two blocks on a CU) and at K = 8"""
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
from scoary_amd.engine import AssociationEngine

SHAPES = len(sys.argv) > 1 and sys.argv[1] == "shapes"
REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 and not SHAPES else 7
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 2
K = 4
REF_BATCH = 256
STRATA = (10, 1000)

if not torch.cuda.is_available():
    sys.exit("bench_gcmh needs an MI355X: there is nothing to time without one")


def other_shapes():
    eng = AssociationEngine(0)
    rng = np.random.default_rng(5)
    G, P, S = 50000, 10000, 10
    for N, K in ((1024, 4), (1280, 4), (2000, 8), (1024, 8)):
        genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
        codes = rng.integers(1, K + 1, (1, N))
        gm = eng.pack_dense(genes)
        plan, cplan = eng.gcmh_plan(codes, rng.integers(0, S, N)), eng.categorical_plan(codes)
        obs, cobs = eng.gcmh(gm, plan), eng.categorical(gm, cplan)
        tg, tc = [], []
        for i in range(WARMUP + 5):
            eng.set_timing(True)
            eng.gcmh_permute(gm, plan, obs, P, 1)
            torch.cuda.synchronize()
            g = eng.kernel_ms("k_gcmh_permute")
            eng.categorical_permute(gm, cplan, cobs["a"], P, 1)
            torch.cuda.synchronize()
            c = eng.kernel_ms("k_cat_permute")
            eng.set_timing(False)
            if i >= WARMUP:
                tg.append(g)
                tc.append(c)
        print("N=%d K=%d G=%d P=%d: k_gcmh_permute median %.3f ms (%.3f-%.3f), k_cat_permute %.3f ms (%.3f-%.3f), "
              "ratio %.3f (n=5)" % (N, K, G, P, statistics.median(tg), min(tg), max(tg), statistics.median(tc), min(tc),
                                    max(tc), statistics.median(tg) / statistics.median(tc)), flush=True)


if SHAPES:
    other_shapes()
    sys.exit(0)
genes, _traits, P, seed = synth.make_config("cfg3", T=1)
G, N = genes.shape
rng = np.random.default_rng(seed + 21)
codes = rng.choice(np.arange(1, K + 1), size=(1, N), p=[0.4, 0.3, 0.2, 0.1])
codes[0, rng.random(N) < 0.01] = 0
eng = AssociationEngine(0)
gm = eng.pack_dense(genes)
cplan = eng.categorical_plan(codes)
cobs = eng.categorical(gm, cplan)
print("date %s  shape G=%d N=%d T=1 K=%d P=%d  n=%d n_k=%s  repeats %d warm-up %d" % (
    datetime.date.today().isoformat(), G, N, K, P, int(cplan.n[0]), cplan.nk_host[0, :K].tolist(), REPEATS, WARMUP),
    flush=True)


def sync_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def timed(fn, kernels):
    eng.set_timing(True)
    try:
        r, ms = sync_ms(fn)
        return (r, ms) + tuple(eng.kernel_ms(k) for k in kernels)
    finally:
        eng.set_timing(False)


def reference(plan, obs):
    """r by fp32 products of the 0/1 matrix with the one-hot class planes of the generator's rows (every partial sum an
    integer below 2^24), then Q of the form in fp64 by elementwise operations in the kernel's order."""
    nc = K - 1
    form, thr = obs["form"][0], obs["thr"][0]
    E, f, invp = form[:, :7], form[:, 7:28], form[:, 28:]
    a_f32 = torch.from_numpy(genes).to(eng.device).to(torch.float32)
    r = torch.zeros(G, dtype=torch.int64, device=eng.device)
    for base in range(0, P, REF_BATCH):
        pb = min(REF_BATCH, P - base)
        rows = eng.gcmh_rows(plan, base, pb, seed)[0]
        y = []
        for i in range(nc):
            plane = (rows == i + 1).to(torch.float32).t().contiguous()
            x = torch.matmul(a_f32, plane).to(torch.float64) - E[:, i:i + 1]
            for j in range(i):
                x = x - f[:, i * (i - 1) // 2 + j:i * (i - 1) // 2 + j + 1] * y[j]
            y.append(x)
        q = torch.zeros((G, pb), dtype=torch.float64, device=eng.device)
        for j in range(nc):
            q = q + (y[j] * y[j]) * invp[:, j:j + 1]
        r += (q >= thr[:, None]).sum(dim=1)
    return r


def line(name, xs):
    print("%-58s median %9.3f ms  min %9.3f  max %9.3f  (n=%d)" % (name, statistics.median(xs), min(xs), max(xs),
                                                                   len(xs)), flush=True)


for S in STRATA:
    strata = rng.integers(0, S, N)
    strata[0] = S - 1
    plan = eng.gcmh_plan(codes, strata)
    obs, obs_ms, seg_ms, ker_ms = timed(lambda: eng.gcmh(gm, plan), ("k_cmh_segments", "k_gcmh_observed"))
    df = obs["df"][0]
    print("S=%d: strata of %d to %d labelled isolates; df 0 / 1 / 2 / 3 on %s genes; k_cmh_segments %.3f ms, "
          "k_gcmh_observed %.3f ms, gcmh() %.3f ms by the host clock" % (
              S, int(plan.nsk_host[0].sum(axis=1).min()), int(plan.nsk_host[0].sum(axis=1).max()),
              " / ".join(str(int((df == d).sum())) for d in range(4)), seg_ms, ker_ms, obs_ms), flush=True)
    r_ref = reference(plan, obs)
    r_ours = eng.gcmh_permute(gm, plan, obs, P, seed)[0].to(torch.int64)
    bad = int((r_ours != r_ref).sum())
    print("S=%d: k_gcmh_permute against the same rule in torch: %d of %d genes differ; r < P on %d genes" % (
        S, bad, G, int((r_ours < P).sum())), flush=True)
    if bad:
        sys.exit("the counts disagree: nothing is timed")
    t = {k: [] for k in ("gstep", "glabels", "gpermute", "cstep", "clabels", "cpermute")}
    for i in range(WARMUP + REPEATS):
        order = ["gcmh", "cat"]
        for which in (order if i % 2 == 0 else order[::-1]):
            if which == "gcmh":
                _r, ms, lab, perm = timed(lambda: eng.gcmh_permute(gm, plan, obs, P, seed),
                                          ("k_vanelteren_labels", "k_gcmh_permute"))
                got = dict(gstep=ms, glabels=lab, gpermute=perm)
            else:
                _r, ms, lab, perm = timed(lambda: eng.categorical_permute(gm, cplan, cobs["a"], P, seed),
                                          ("k_ranksum_labels", "k_cat_permute"))
                got = dict(cstep=ms, clabels=lab, cpermute=perm)
            if i >= WARMUP:
                for k, v in got.items():
                    t[k].append(v)
    line("S=%d k_vanelteren_labels (generator, plain rows)" % S, t["glabels"])
    line("S=%d k_gcmh_permute" % S, t["gpermute"])
    line("S=%d gcmh_permute (whole step, host clock)" % S, t["gstep"])
    line("S=%d k_ranksum_labels (S20's generator)" % S, t["clabels"])
    line("S=%d k_cat_permute (S20's kernel)" % S, t["cpermute"])
    line("S=%d categorical_permute (S20's step, host clock)" % S, t["cstep"])
    med = {k: statistics.median(v) for k, v in t.items()}
    print("S=%d: k_gcmh_permute / k_cat_permute = %.3f (k_cat_permute's spread %.3f ms, %.1f %% of its median); "
          "gcmh_permute / categorical_permute = %.3f (that step's spread %.3f ms, %.1f %%)" % (
              S, med["gpermute"] / med["cpermute"], max(t["cpermute"]) - min(t["cpermute"]),
              100.0 * (max(t["cpermute"]) - min(t["cpermute"])) / med["cpermute"], med["gstep"] / med["cstep"],
              max(t["cstep"]) - min(t["cstep"]), 100.0 * (max(t["cstep"]) - min(t["cstep"])) / med["cstep"]),
          flush=True)
try:
    import __graft_entry__ as ge
    with open(ge.HIP_RESOURCES) as f:
        res = json.load(f)
    for name, fields in res.items():
        for kernel in ("k_gcmh_permute", "k_gcmh_observed", "k_cat_permute"):
            if kernel in name:
                print("%s resources: " % kernel + ", ".join("%s %s" % kv for kv in sorted(fields.items())), flush=True)
except (OSError, ImportError, ValueError):
    print("kernel resources: the build's report was not found", flush=True)
