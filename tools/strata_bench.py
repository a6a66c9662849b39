"""Labels shuffled within strata (spec S9) at cfg3's shape on one MI355X: k_labels_strata alone (set_timing /
kernel_ms) and the whole associate() step, for S in {1, 8, 64, 256} equal-sized strata in index blocks and for S = 8
assigned at random, each against the unstratified values of the same run (the variants alternate inside every
repeat).  The stratified step may cost at most 10 % more than the plain step.  Raw lines on stdout
(profiles/strata_generator.txt).
    python tools/strata_bench.py [repeats]"""
import os, sys, time, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from scoary_amd import synth
from scoary_amd.engine import AssociationEngine, pack_bits_rows

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
genes, traits, P, seed = synth.make_config("cfg3")
G, N = genes.shape; T = traits.shape[0]
eng = AssociationEngine(0)
gm = eng.pack_dense(genes)
trv = eng.vecrows(pack_bits_rows((traits == 1).astype(np.uint8)), N)
mkv = eng.vecrows(pack_bits_rows((traits != 2).astype(np.uint8)), N)
plan = eng.trait_plan(trv, mkv, N)
eng.build_lists(gm)
ws = eng.workspace(gm, T, P)
print("shape G=%d N=%d T=%d P=%d repeats %d" % (G, N, T, P, REPEATS), flush=True)

rng = np.random.default_rng(1)
variants = [("plain", None)]
for S in (1, 8, 64, 256):
    variants.append(("S=%d blocks" % S, eng.strata_plan(np.arange(N) * S // N, trv, mkv, N)))
variants.append(("S=8 random", eng.strata_plan(rng.integers(0, 8, N), trv, mkv, N)))
for name, sp in variants[1:]:
    print("%s: sizes %d..%d" % (name, sp.sizes.min(), sp.sizes.max()), flush=True)


def step(sp):
    return eng.associate(gm, trv, mkv, permutations=P, seed=seed, plan=plan, workspace=ws, graph=False, strata=sp)


def kernel_ms(sp):
    """The generator alone: one batch of label tiles, timed by the library's own events."""
    nb = min(ws.batch, P)
    eng.set_timing(True)
    try:
        eng.perm_generate_tiles(mkv, plan.margins, N, nb, 0, seed, out=ws.tiles, strata=sp)
        return eng.kernel_ms("k_perm_generate_tiles_strata" if sp is not None else "k_perm_generate_tiles")
    finally:
        eng.set_timing(False)


for _name, sp in variants:                       # warm-up: code objects, LDS opt-in, side stream
    step(sp); kernel_ms(sp)
torch.cuda.synchronize()
kern = {name: [] for name, _ in variants}
whole = {name: [] for name, _ in variants}
for i in range(REPEATS):
    order = variants if i % 2 == 0 else variants[::-1]
    for name, sp in order:
        kern[name].append(kernel_ms(sp))
    for name, sp in order:
        torch.cuda.synchronize(); t0 = time.perf_counter(); step(sp); torch.cuda.synchronize()
        whole[name].append((time.perf_counter() - t0) * 1e3)
base_k, base_w = statistics.median(kern["plain"]), statistics.median(whole["plain"])
worst = 0.0
for name, _sp in variants:
    k, w = statistics.median(kern[name]), statistics.median(whole[name])
    worst = max(worst, w / base_w)
    print("%-12s generator median %.4f ms (min %.4f max %.4f, x%.2f)   step median %.4f ms (min %.4f max %.4f, x%.3f)"
          % (name, k, min(kern[name]), max(kern[name]), k / base_k, w, min(whole[name]), max(whole[name]), w / base_w),
          flush=True)
print("WORST step ratio %.3f (bound 1.10): %s" % (worst, "within" if worst <= 1.10 else "MISSED"), flush=True)
