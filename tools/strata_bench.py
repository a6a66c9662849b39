"""Labels shuffled within strata (spec S9) at cfg3's shape on one MI355X: k_labels_strata alone (set_timing /
kernel_ms) and the whole associate() step, for S in {1, 8, 64, 256} equal-sized strata in index blocks and for S = 8
assigned at random, each against the unstratified values of the same run (the variants alternate inside every
repeat).  The stratified step may cost at most 10 % more than the plain step.  After these, the kernel instances
cfg3's tiles do not reach: the bit-row generators (k_perm_generate / k_perm_generate_strata, one batch of
perm_batch(T, N, P) rows at cfg3's shape) and the one-column tile kernels (N = 2000, T = 1, P = 8192: 16 tiles of
8 columns, too few blocks for two columns each).  Raw lines on stdout (profiles/strata_generator.txt).
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


def rows_ms(sp):
    """One batch of label rows (k_labels<1, 1> / k_labels_strata<1, 1>)."""
    eng.set_timing(True)
    try:
        eng.perm_generate(mkv, plan.margins, N, rows.shape[1], 0, seed, out=rows, strata=sp)
        return eng.kernel_ms("k_perm_generate_strata" if sp is not None else "k_perm_generate")
    finally:
        eng.set_timing(False)


# the one-column tile kernels (k_labels<1, 0> / k_labels_strata<1, 0>): a launch too small for two columns per block
N1, P1 = 2000, 8192
t1 = (rng.random((1, N1)) < 0.4).astype(np.uint8)
trv1 = eng.vecrows(pack_bits_rows(t1), N1)
mkv1 = eng.vecrows(pack_bits_rows(np.ones_like(t1)), N1)
plan1 = eng.trait_plan(trv1, mkv1, N1)
tiles1 = torch.empty(int(eng.lib.scoary_list_tiles_words(N1, P1, 1)), dtype=torch.int32, device=eng.device)
assert eng.tiles_per_batch(N1, P1, 1)[0] * (eng.list_params(N1)[0] // 2) < \
    2 * torch.cuda.get_device_properties(0).multi_processor_count
small = [("plain", None), ("S=8 blocks", eng.strata_plan(np.arange(N1) * 8 // N1, trv1, mkv1, N1))]


def one_column_ms(sp):
    eng.set_timing(True)
    try:
        eng.perm_generate_tiles(mkv1, plan1.margins, N1, P1, 0, seed, out=tiles1, strata=sp)
        return eng.kernel_ms("k_perm_generate_tiles_strata" if sp is not None else "k_perm_generate_tiles")
    finally:
        eng.set_timing(False)


rows = torch.empty((T, eng.perm_batch(T, N, P), eng.row_words(N)), dtype=torch.int32, device=eng.device)
for _name, sp in variants:                       # warm-up: code objects, LDS opt-in, side stream
    step(sp); kernel_ms(sp); rows_ms(sp)
for _name, sp in small:
    one_column_ms(sp)
torch.cuda.synchronize()
kern = {name: [] for name, _ in variants}
rowk = {name: [] for name, _ in variants}
onek = {name: [] for name, _ in small}
whole = {name: [] for name, _ in variants}
for i in range(REPEATS):
    order = variants if i % 2 == 0 else variants[::-1]
    for name, sp in order:
        kern[name].append(kernel_ms(sp))
    for name, sp in order:
        torch.cuda.synchronize(); t0 = time.perf_counter(); step(sp); torch.cuda.synchronize()
        whole[name].append((time.perf_counter() - t0) * 1e3)
    for name, sp in order:
        rowk[name].append(rows_ms(sp))
    for name, sp in small if i % 2 == 0 else small[::-1]:
        onek[name].append(one_column_ms(sp))
base_k, base_w = statistics.median(kern["plain"]), statistics.median(whole["plain"])
worst = 0.0
for name, _sp in variants:
    k, w = statistics.median(kern[name]), statistics.median(whole[name])
    worst = max(worst, w / base_w)
    print("%-12s generator median %.4f ms (min %.4f max %.4f, x%.2f)   step median %.4f ms (min %.4f max %.4f, x%.3f)"
          % (name, k, min(kern[name]), max(kern[name]), k / base_k, w, min(whole[name]), max(whole[name]), w / base_w),
          flush=True)
print("WORST step ratio %.3f (bound 1.10): %s" % (worst, "within" if worst <= 1.10 else "MISSED"), flush=True)
for title, res in (("rows", rowk), ("one column", onek)):
    for name, v in res.items():
        print("%-12s %s median %.4f ms (min %.4f max %.4f)" % (name, title, statistics.median(v), min(v), max(v)),
              flush=True)
