"""The Cochran-Mantel-Haenszel test (spec S10) at cfg3's shape on one MI355X with S = 50 strata: k_cmh alone
(set_timing / kernel_ms, with k_cmh_segments beside it) for strata assigned at random (interleaved: one segment per
isolate) and in index blocks (contiguous: about W + S segments), and the whole associate(strata=..., permutations =
10 000) step with cmh=True beside the same step with cmh=False, the variants alternating inside every repeat.  The
second exceedance pass is expected to roughly double the permutation time; that is an expectation to record, not a
bound.  Raw lines on stdout (profiles/cmh.txt).
    python tools/cmh_bench.py [repeats]"""
import os, sys, time, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from scoary_amd import synth
from scoary_amd.engine import AssociationEngine, pack_bits_rows

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
S = 50
genes, traits, P, seed = synth.make_config("cfg3")
G, N = genes.shape; T = traits.shape[0]
eng = AssociationEngine(0)
gm = eng.pack_dense(genes)
trv = eng.vecrows(pack_bits_rows((traits == 1).astype(np.uint8)), N)
mkv = eng.vecrows(pack_bits_rows((traits != 2).astype(np.uint8)), N)
plan = eng.trait_plan(trv, mkv, N)
eng.build_lists(gm)
ws = eng.workspace(gm, T, P)
print("shape G=%d N=%d T=%d P=%d S=%d repeats %d" % (G, N, T, P, S, REPEATS), flush=True)

rng = np.random.default_rng(1)
variants = [("interleaved", eng.strata_plan(rng.integers(0, S, N), trv, mkv, N, S=S)),
            ("contiguous", eng.strata_plan(np.arange(N) * S // N, trv, mkv, N, S=S))]


def kernel_ms(sp):
    eng.set_timing(True)
    try:
        eng.cmh(gm, trv, mkv, sp)
        return eng.kernel_ms("k_cmh"), eng.kernel_ms("k_cmh_segments")
    finally:
        eng.set_timing(False)


def step(sp, cmh):
    return eng.associate(gm, trv, mkv, permutations=P, seed=seed, plan=plan, workspace=ws, graph=False, strata=sp,
                         cmh=cmh)


for _name, sp in variants:                       # warm-up: code objects, LDS opt-in, side stream
    kernel_ms(sp); step(sp, False); step(sp, True)
torch.cuda.synchronize()
kern = {name: [] for name, _ in variants}
segk = {name: [] for name, _ in variants}
whole = {(name, c): [] for name, _ in variants for c in (False, True)}
for i in range(REPEATS):
    order = variants if i % 2 == 0 else variants[::-1]
    for name, sp in order:
        k, s = kernel_ms(sp)
        kern[name].append(k); segk[name].append(s)
    for name, sp in order:
        for c in ((False, True) if i % 2 == 0 else (True, False)):
            torch.cuda.synchronize(); t0 = time.perf_counter(); step(sp, c); torch.cuda.synchronize()
            whole[(name, c)].append((time.perf_counter() - t0) * 1e3)
for name, sp in variants:
    k, s = kern[name], segk[name]
    print("%-12s k_cmh median %.4f ms (min %.4f max %.4f)   k_cmh_segments median %.4f ms (min %.4f max %.4f)"
          % (name, statistics.median(k), min(k), max(k), statistics.median(s), min(s), max(s)), flush=True)
for name, sp in variants:
    w0, w1 = whole[(name, False)], whole[(name, True)]
    m0, m1 = statistics.median(w0), statistics.median(w1)
    print("%-12s step cmh=False median %.4f ms (min %.4f max %.4f)   cmh=True median %.4f ms (min %.4f max %.4f)   "
          "x%.3f" % (name, m0, min(w0), max(w0), m1, min(w1), max(w1), m1 / m0), flush=True)
