"""The Breslow-Day / Tarone homogeneity test (spec S14) at cfg3's shape on one MI355X: k_cmh_homog beside k_cmh in the
same process (set_timing / kernel_ms), the two alternating inside every repeat, for S = 50 and S = 256 strata assigned
at random (interleaved: one segment per isolate) and in index blocks (contiguous: about W + S segments).  The number
to read is the ratio to k_cmh on the same shape.  Raw lines on stdout (profiles/cmh_homog.txt).
    python tools/cmh_homog_bench.py [repeats]"""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from scoary_amd import synth
from scoary_amd.engine import AssociationEngine, pack_bits_rows

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
genes, traits, _P, _seed = synth.make_config("cfg3")
G, N = genes.shape; T = traits.shape[0]
eng = AssociationEngine(0)
gm = eng.pack_dense(genes)
trv = eng.vecrows(pack_bits_rows((traits == 1).astype(np.uint8)), N)
mkv = eng.vecrows(pack_bits_rows((traits != 2).astype(np.uint8)), N)
print("shape G=%d N=%d T=%d repeats %d" % (G, N, T, REPEATS), flush=True)


def timed(name, fn):
    eng.set_timing(True)
    try:
        out = fn()
        return out, eng.kernel_ms(name)
    finally:
        eng.set_timing(False)


for S in (50, 256):
    rng = np.random.default_rng(1)
    variants = [("interleaved", eng.strata_plan(rng.integers(0, S, N), trv, mkv, N, S=S)),
                ("contiguous", eng.strata_plan(np.arange(N) * S // N, trv, mkv, N, S=S))]
    for name, sp in variants:
        res = eng.cmh(gm, trv, mkv, sp)
        hom = eng.cmh_homogeneity(gm, trv, mkv, sp, res)                       # warm-up
        torch.cuda.synchronize()
        df = hom["df"]
        print("S=%-4d %-12s defined rows %d of %d, df median %d max %d" % (
            S, name, int((df > 0).sum()), df.numel(), int(df[df > 0].median()) if (df > 0).any() else 0, int(df.max())),
            flush=True)
        cmh_ms, homog_ms = [], []
        for i in range(REPEATS):
            for which in ((0, 1) if i % 2 == 0 else (1, 0)):
                if which == 0:
                    cmh_ms.append(timed("k_cmh", lambda: eng.cmh(gm, trv, mkv, sp))[1])
                else:
                    homog_ms.append(timed("k_cmh_homog", lambda: eng.cmh_homogeneity(gm, trv, mkv, sp, res))[1])
        mc, mh = statistics.median(cmh_ms), statistics.median(homog_ms)
        print("S=%-4d %-12s k_cmh median %.4f ms (min %.4f max %.4f)   k_cmh_homog median %.4f ms (min %.4f max %.4f)   "
              "x%.3f" % (S, name, mc, min(cmh_ms), max(cmh_ms), mh, min(homog_ms), max(homog_ms), mh / mc), flush=True)
