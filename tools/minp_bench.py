"""Westfall-Young minP (spec S7) at cfg3's shape on one MI355X: the p tables (build time, bytes), k_permute_minp
against the dense permutation kernel (same process, alternating order; the kernel's ceiling is 2x the dense median),
and the whole associate(fwer=True) step next to the plain step.  Raw lines on stdout (profiles/r10_minp.txt).
    python tools/minp_bench.py"""
import os, sys, time, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from scoary_amd import synth
from scoary_amd.engine import AssociationEngine, pack_bits_rows

genes, traits, P, seed = synth.make_config("cfg3")
G, N = genes.shape; T = traits.shape[0]
eng = AssociationEngine(0)
gm = eng.pack_dense(genes)
trv = eng.vecrows(pack_bits_rows((traits == 1).astype(np.uint8)), N)
mkv = eng.vecrows(pack_bits_rows((traits != 2).astype(np.uint8)), N)
plan = eng.trait_plan(trv, mkv, N)
print("shape G=%d N=%d T=%d P=%d" % (G, N, T, P), flush=True)
res = eng.associate(gm, trv, mkv, permutations=0, plan=plan)
torch.cuda.synchronize()
# tables
for i in range(3):
    eng.set_timing(True)
    t0 = time.perf_counter()
    tables = eng.minp_tables(res["counts"])
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    print("tables run %d: entries %d bytes %d k_minp_plan %.3f ms k_minp_fill %.3f ms (k_fisher inside, avg per chunk %.3f ms) wall %.3f ms"
          % (i, tables.entries, tables.entries * 8, eng.kernel_ms("k_minp_plan"), eng.kernel_ms("k_minp_fill"),
             eng.kernel_ms("k_fisher"), wall), flush=True)
    eng.set_timing(False)
    if i < 2:
        del tables
Wp = eng.row_words(N)
perms = eng.perm_generate(mkv, res["margins"], N, P, 0, seed)
crit = eng.fisher(res["counts"], want_crit=True)[2]
r = torch.zeros((T, G), dtype=torch.int32, device=eng.device)
minp = torch.ones((T, P), dtype=torch.float64, device=eng.device)
dense_ms, minp_ms = [], []
for i in range(7):
    for which in (("dense", "minp") if i % 2 == 0 else ("minp", "dense")):
        eng.set_timing(True)
        if which == "dense":
            eng.permute(gm, perms, crit, r)
            ms = eng.kernel_ms("k_permute"); dense_ms.append(ms)
        else:
            eng.permute_minp(gm, perms, tables, minp)
            ms = eng.kernel_ms("k_permute_minp"); minp_ms.append(ms)
        eng.set_timing(False)
        print("kernel pair %d %s %.3f ms" % (i, which, ms), flush=True)
# the issue's form of the dense figure: associate(use_lists=False) with set_timing / kernel_ms
for i in range(5):
    eng.set_timing(True)
    eng.associate(gm, trv, mkv, permutations=P, seed=seed, use_lists=False, plan=plan)
    print("associate(use_lists=False) run %d k_permute %.3f ms" % (i, eng.kernel_ms("k_permute")), flush=True)
    eng.set_timing(False)
md, mm = statistics.median(dense_ms), statistics.median(minp_ms)
print("MEDIAN k_permute (dense) %.3f ms  k_permute_minp %.3f ms  ratio %.3f (ceiling 2.0)" % (md, mm, mm / md), flush=True)
# whole step: plain (list path) against fwer
eng.build_lists(gm)
def timed(fn, n=5):
    out = []
    for _ in range(n):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out
plain = lambda: eng.associate(gm, trv, mkv, permutations=P, seed=seed, plan=plan, graph=False)
fw = lambda: eng.associate(gm, trv, mkv, permutations=P, seed=seed, plan=plan, fwer=True)     # tables kept with gm
fw_cold = lambda: eng.associate(gm, trv, mkv, permutations=P, seed=seed, fwer=True)         # tables rebuilt per call
del tables
plain(); fw_cold(); fw()
a, c, b = timed(plain), timed(fw_cold), timed(fw)
print("whole step plain (lists) ms:", " ".join("%.3f" % x for x in a), "median %.3f" % statistics.median(a))
print("whole step fwer, tables rebuilt (no plan) ms:", " ".join("%.3f" % x for x in c), "median %.3f" % statistics.median(c))
print("whole step fwer, tables cached (plan) ms:", " ".join("%.3f" % x for x in b), "median %.3f" % statistics.median(b))
out = fw()
print("minp[0][:4]", out["minp"][0, :4].tolist(), "r_fwer<P per trait", [(int((out["r_fwer"][t] < P).sum())) for t in range(T)])
