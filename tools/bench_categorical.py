"""The categorical permutation step (spec S20) at cfg3's geometry with one trait of K = 4 classes on one MI355X:
G = 50 000 genes (Roary-like frequencies from synth), N = 2000 isolates, P = 10 000 label permutations.

Timed, every repeat in the same process, the variants alternating inside a repeat:
  * k_ranksum_labels (the generator, plain rows) and k_cat_permute, each by device events (set_timing / kernel_ms),
    and the whole step engine.categorical_permute by a host clock around a device synchronise;
  * what a user does today: the trait cut into K one-vs-rest binary traits (an isolate without a label missing in all
    of them) and their permutation step through associate() on the same genes, list path, one call of K traits.
Before anything is timed the counts of k_cat_permute are held to an exact fp32 formulation of the same rule on the
generator's rows (a_k by matrix products, sum a_k^2 L / n_k in int64: L is small at this shape).
Reported: median, min and max of each, the generator's share of the step, (set bit, permutation) pairs walked per
second, and the ratio of the step to the one-vs-rest workaround -- reported, not gated.  Raw lines on stdout
(profiles/categorical.txt).
    python tools/bench_categorical.py [repeats] [warmup]
    python tools/bench_categorical.py once        one untimed step and nothing else: the run a counter pass wraps"""
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
from scoary_amd.engine import AssociationEngine, pack_bits_rows

ONCE = len(sys.argv) > 1 and sys.argv[1] == "once"
REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 and not ONCE else 7
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 2
K = 4
REF_BATCH = 1024

if not torch.cuda.is_available():
    sys.exit("bench_categorical needs an MI355X: there is nothing to time without one")
genes, _traits, P, seed = synth.make_config("cfg3", T=1)
G, N = genes.shape
rng = np.random.default_rng(seed + 20)
codes = rng.choice(np.arange(1, K + 1), size=(1, N), p=[0.4, 0.3, 0.2, 0.1])
codes[0, rng.random(N) < 0.01] = 0
eng = AssociationEngine(0)
gm = eng.pack_dense(genes)
plan = eng.categorical_plan(codes)
obs = eng.categorical(gm, plan)
a_obs = obs["a"]
m = genes[:, codes[0] != 0].sum(axis=1).astype(np.int64)
walked = int(np.minimum(m, int(plan.n[0]) - m).sum())          # set bits walked per permutation, over all genes
if ONCE:
    eng.categorical_permute(gm, plan, a_obs, P, seed)
    torch.cuda.synchronize()
    sys.exit(0)
print("date %s  shape G=%d N=%d T=1 K=%d P=%d  n=%d n_k=%s  set bits walked per permutation %d (%.1f a gene)  "
      "repeats %d warm-up %d" % (datetime.date.today().isoformat(), G, N, K, P, int(plan.n[0]),
                                 plan.nk_host[0, :K].tolist(), walked, walked / G, REPEATS, WARMUP), flush=True)


def sync_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def ours():
    eng.set_timing(True)
    try:
        r, ms = sync_ms(lambda: eng.categorical_permute(gm, plan, a_obs, P, seed))
        return r, ms, eng.kernel_ms("k_ranksum_labels"), eng.kernel_ms("k_cat_permute")
    finally:
        eng.set_timing(False)


def exact_reference():
    """r by fp32 products of the 0/1 matrix with the one-hot class planes of the generator's rows (every partial sum
    an integer below 2^24), then sum a_k^2 w_k in int64 (that K N^2 max w_k stays below 2^63 is checked)."""
    w = [int(x) for x in plan.weights[0]]
    assert K * N * N * max(w) < 1 << 63
    wt = torch.tensor(w[:K], dtype=torch.int64, device=eng.device)
    a_f32 = torch.from_numpy(genes).to(eng.device).to(torch.float32)
    s_obs = (a_obs[0, :, :K].to(torch.int64) ** 2 * wt).sum(dim=1)
    r = torch.zeros(G, dtype=torch.int64, device=eng.device)
    for base in range(0, P, REF_BATCH):
        pb = min(REF_BATCH, P - base)
        rows = eng.categorical_rows(plan, base, pb, seed)[0]
        s = torch.zeros((G, pb), dtype=torch.int64, device=eng.device)
        for k in range(K):
            plane = (rows == k + 1).to(torch.float32).t().contiguous()
            s += torch.matmul(a_f32, plane).to(torch.int64) ** 2 * wt[k]
        r += (s >= s_obs[:, None]).sum(dim=1)
    return r


r_ref = exact_reference()
r_ours = ours()[0][0].to(torch.int64)
bad = int((r_ours != r_ref).sum())
print("k_cat_permute against the exact fp32 formulation: %d of %d genes differ; r < P on %d genes" % (
    bad, G, int((r_ours < P).sum())), flush=True)
if bad:
    sys.exit("the counts disagree: nothing is timed")

# the workaround: K one-vs-rest binary traits through associate(), list path
ovr = np.stack([np.where(codes[0] == 0, 2, (codes[0] == k + 1).astype(np.int64)) for k in range(K)]).astype(np.uint8)
trv = eng.vecrows(pack_bits_rows((ovr == 1).astype(np.uint8)), N)
mkv = eng.vecrows(pack_bits_rows((ovr != 2).astype(np.uint8)), N)
eng.build_lists(gm)


def one_vs_rest():
    return sync_ms(lambda: eng.associate(gm, trv, mkv, permutations=P, seed=seed, use_lists=True))[1]


t = {k: [] for k in ("step", "labels", "permute", "ovr")}
for i in range(WARMUP + REPEATS):
    keep = i >= WARMUP
    order = ["ours", "ovr"]
    for which in (order if i % 2 == 0 else order[::-1]):
        if which == "ours":
            _r, ms, lab, perm = ours()
            got = dict(step=ms, labels=lab, permute=perm)
        else:
            got = dict(ovr=one_vs_rest())
        if keep:
            for k, v in got.items():
                t[k].append(v)


def line(name, xs):
    print("%-52s median %9.3f ms  min %9.3f  max %9.3f  (n=%d)" % (name, statistics.median(xs), min(xs), max(xs),
                                                                   len(xs)), flush=True)


line("k_ranksum_labels (generator, plain rows)", t["labels"])
line("k_cat_permute (per step = per trait here)", t["permute"])
line("categorical_permute (whole step, host clock)", t["step"])
line("one-vs-rest: associate(), %d binary traits, lists" % K, t["ovr"])
perm, step, ovr_ms = (statistics.median(t[k]) for k in ("permute", "step", "ovr"))
print("generator's share of the step: %.1f %%" % (100.0 * statistics.median(t["labels"]) / step), flush=True)
print("k_cat_permute: %.3g (set bit, permutation) pairs per second (%d x P = %.3g over the median)" % (
    walked * float(P) / (perm * 1e-3), walked, walked * float(P)), flush=True)
spread = max(t["ovr"]) - min(t["ovr"])
print("categorical_permute / one-vs-rest step = %.3f (k_cat_permute alone / one-vs-rest = %.3f); the one-vs-rest "
      "step's run-to-run spread is %.3f ms (%.1f %% of its median)" % (step / ovr_ms, perm / ovr_ms, spread,
                                                                      100.0 * spread / ovr_ms), flush=True)
try:
    import __graft_entry__ as ge
    with open(ge.HIP_RESOURCES) as f:
        res = json.load(f)
    for name, fields in res.items():
        if "k_cat_permute" in name:
            print("k_cat_permute resources: " + ", ".join("%s %s" % kv for kv in sorted(fields.items())), flush=True)
except (OSError, ImportError, ValueError):
    print("k_cat_permute resources: the build's report was not found", flush=True)
