"""Westfall-Young step-down minP (spec S8) at cfg3's shape on one MI355X, p tables cached with the gene matrix:
the kernels of scoary_permute_stepdown next to k_permute_minp (same process, same label rows, alternating order,
hipEvent pairs), and the whole associate(stepdown=True) step next to associate(fwer=True), alternated after both
were warmed up.  SCOARY_HIP_LIB selects another build of the library (tools/build_alt.sh), for A/B runs of kernel
variants.  Raw lines on stdout (profiles/r13_stepdown.txt).
    python tools/stepdown_bench.py [--steps-only N]      (--steps-only: N alternated whole steps, for a kernel trace)"""
import os, sys, time, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from scoary_amd import synth, _abi
from scoary_amd.engine import AssociationEngine, pack_bits_rows

steps_only = int(sys.argv[sys.argv.index("--steps-only") + 1]) if "--steps-only" in sys.argv else 0
genes, traits, P, seed = synth.make_config("cfg3")
G, N = genes.shape; T = traits.shape[0]
eng = AssociationEngine(0)
gm = eng.pack_dense(genes)
trv = eng.vecrows(pack_bits_rows((traits == 1).astype(np.uint8)), N)
mkv = eng.vecrows(pack_bits_rows((traits != 2).astype(np.uint8)), N)
plan = eng.trait_plan(trv, mkv, N)
print("library %s" % _abi.LIB_PATH)
print("shape G=%d N=%d T=%d P=%d nch=%d scratch %.1f MB" % (
    G, N, T, P, eng.stepdown_chunks(G, T, P), eng.lib.scoary_stepdown_scratch_bytes(eng.h, G, T, N, P) / 1e6), flush=True)
eng.build_lists(gm)
fw = lambda: eng.associate(gm, trv, mkv, permutations=P, seed=seed, plan=plan, fwer=True)
sd = lambda: eng.associate(gm, trv, mkv, permutations=P, seed=seed, plan=plan, stepdown=True)
both = lambda: eng.associate(gm, trv, mkv, permutations=P, seed=seed, plan=plan, fwer=True, stepdown=True)
fw(); sd(); fw(); sd(); both()                       # tables built once (kept with gm), both paths warm
torch.cuda.synchronize()
if steps_only:
    for i in range(steps_only):
        fw(); sd()
    torch.cuda.synchronize()
    sys.exit(0)

# 1. kernels
res = eng.associate(gm, trv, mkv, permutations=0, plan=plan)
tables = gm.minp_cache["tables"]
perms = eng.perm_generate(mkv, res["margins"], N, P, 0, seed)
ps, order = torch.sort(res["p"], dim=1, stable=True)
ps, order = ps.contiguous(), order.to(torch.int32).contiguous()
c = torch.zeros((T, G), dtype=torch.int32, device=eng.device)
minp = torch.ones((T, P), dtype=torch.float64, device=eng.device)
names = ("k_stepdown_prep", "k_stepdown_minp_cells", "k_stepdown_minp_count", "k_stepdown_sum")
minp_ms, sd_ms = [], {n: [] for n in names}
for i in range(7):
    for which in (("minp", "stepdown") if i % 2 == 0 else ("stepdown", "minp")):
        eng.set_timing(True)
        if which == "minp":
            eng.permute_minp(gm, perms, tables, minp)
            ms = eng.kernel_ms("k_permute_minp"); minp_ms.append(ms)
            print("kernel pair %d k_permute_minp %.3f ms" % (i, ms), flush=True)
        else:
            eng.permute_stepdown(gm, perms, tables, order, ps, c, minp=minp)
            got = [eng.kernel_ms(n) for n in names]
            for n, ms in zip(names, got):
                sd_ms[n].append(ms)
            print("kernel pair %d stepdown %s total %.3f ms" % (
                i, " ".join("%s %.3f" % (n, ms) for n, ms in zip(names, got)), sum(got)), flush=True)
        eng.set_timing(False)
mm = statistics.median(minp_ms)
med = {n: statistics.median(v) for n, v in sd_ms.items()}
tot = sum(med.values())
print("MEDIAN k_permute_minp %.3f ms | %s | step-down kernels %.3f ms  ratio %.3f (expectation ~2)" % (
    mm, "  ".join("%s %.3f" % kv for kv in med.items()), tot, tot / mm), flush=True)


# 2. whole steps, alternated
def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3
a, b, d = [], [], []
for i in range(7):
    if i % 2 == 0:
        a.append(timed(fw)); b.append(timed(sd))
    else:
        b.append(timed(sd)); a.append(timed(fw))
    d.append(timed(both))
print("whole step fwer, tables cached ms:", " ".join("%.3f" % x for x in a), "median %.3f" % statistics.median(a))
print("whole step stepdown, tables cached ms:", " ".join("%.3f" % x for x in b), "median %.3f" % statistics.median(b))
print("whole step fwer + stepdown, tables cached ms:", " ".join("%.3f" % x for x in d), "median %.3f" % statistics.median(d))
print("step ratio stepdown / fwer %.3f" % (statistics.median(b) / statistics.median(a)))
out = both()
print("genes with r_sd < r_fwer per trait", [int((out["r_fwer_sd"][t] < out["r_fwer"][t]).sum()) for t in range(T)],
      "r_sd > r_fwer anywhere:", bool((out["r_fwer_sd"] > out["r_fwer"]).any()),
      "r_sd<P per trait", [int((out["r_fwer_sd"][t] < P).sum()) for t in range(T)])
