"""The exact conditional test over the strata (spec S12) at cfg3's shape on one MI355X: k_cmh_exact with and without
the table (set_timing / kernel_ms), for S = 50 strata assigned at random (interleaved: one segment per isolate) and
in index blocks (contiguous), and for S = 256 -- beside the yardsticks a reader will compare with, timed in the same
process with the variants alternating inside every repeat: the S11 tables of the same strata (k_cmh_minp_plan +
k_cmh_minp_fill) and Fisher's table build (k_minp_plan + k_minp_fill, S7).  Raw lines on stdout
(profiles/cmh_exact.txt).
    python tools/cmh_exact_bench.py [repeats]"""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from scoary_amd import synth
from scoary_amd.engine import AssociationEngine, pack_bits_rows

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
genes, traits, P, seed = synth.make_config("cfg3")
G, N = genes.shape; T = traits.shape[0]
eng = AssociationEngine(0)
gm = eng.pack_dense(genes)
trv = eng.vecrows(pack_bits_rows((traits == 1).astype(np.uint8)), N)
mkv = eng.vecrows(pack_bits_rows((traits != 2).astype(np.uint8)), N)
plan = eng.trait_plan(trv, mkv, N)
res = eng.associate(gm, trv, mkv, permutations=0, plan=plan)
print("shape G=%d N=%d T=%d repeats %d" % (G, N, T, REPEATS), flush=True)

rng = np.random.default_rng(1)
variants = [("S=50 interleaved", eng.strata_plan(rng.integers(0, 50, N), trv, mkv, N, S=50)),
            ("S=50 contiguous", eng.strata_plan(np.arange(N) * 50 // N, trv, mkv, N, S=50)),
            ("S=256 interleaved", eng.strata_plan(rng.integers(0, 256, N), trv, mkv, N, S=256)),
            ("S=256 contiguous", eng.strata_plan(np.arange(N) * 256 // N, trv, mkv, N, S=256))]


def timed(names, fn):
    eng.set_timing(True)
    try:
        out = fn()
        return out, [eng.kernel_ms(n) for n in names]
    finally:
        eng.set_timing(False)


cm = {name: eng.cmh(gm, trv, mkv, sp) for name, sp in variants}
runs = {"exact": lambda n, sp: eng.cmh_exact(gm, mkv, sp, cm[n]),
        "exact+table": lambda n, sp: eng.cmh_exact(gm, mkv, sp, cm[n], tables=True),
        "cmh tables": lambda n, sp: eng.cmh_tables(gm, mkv, sp, cm[n]),
        "fisher tables": lambda n, sp: eng.minp_tables(res["counts"])}
events = {"exact": ("k_cmh_exact", "k_cmh_minp_plan"), "exact+table": ("k_cmh_exact", "k_cmh_minp_plan"),
          "cmh tables": ("k_cmh_minp_fill", "k_cmh_minp_plan"), "fisher tables": ("k_minp_fill", "k_minp_plan")}
for name, sp in variants:
    t = runs["exact+table"](name, sp)["tables"]
    print("%-18s entries %.1f M (%.1f per pair, longest %d)"
          % (name, t.entries / 1e6, t.entries / (T * G), int((t.off[1:] - t.off[:-1]).max())), flush=True)
    del t
    for kind in runs:
        runs[kind](name, sp)
torch.cuda.synchronize()
ms = {(name, kind): [] for name, _ in variants for kind in runs}
for i in range(REPEATS):
    for name, sp in (variants if i % 2 == 0 else variants[::-1]):
        for kind in (list(runs) if i % 2 == 0 else list(runs)[::-1]):
            out, got = timed(events[kind], lambda: runs[kind](name, sp))
            ms[(name, kind)].append(got)
            del out
for name, _sp in variants:
    for kind in runs:
        main = [a for a, _b in ms[(name, kind)]]
        plan_ms = [b for _a, b in ms[(name, kind)]]
        print("%-18s %-13s %-16s median %.3f ms (min %.3f max %.3f)   %-16s median %.3f ms"
              % (name, kind, events[kind][0], statistics.median(main), min(main), max(main), events[kind][1],
                 statistics.median(plan_ms)), flush=True)
