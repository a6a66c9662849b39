"""The Cochran-Mantel-Haenszel test (spec S10) at cfg3's shape on one MI355X with S = 50 strata: k_cmh alone
(set_timing / kernel_ms, with k_cmh_segments beside it) for strata assigned at random (interleaved: one segment per
isolate) and in index blocks (contiguous: about W + S segments), and the whole associate(strata=..., permutations =
10 000) step with cmh=True beside the same step with cmh=False, the variants alternating inside every repeat.  The
second exceedance pass is expected to roughly double the permutation time; that is an expectation to record, not a
bound.  Raw lines on stdout (profiles/cmh.txt).
    python tools/cmh_bench.py [repeats]
With ``wy`` after the repeats: the Westfall-Young passes over the CMH statistic (spec S11) instead -- the table plan and
fill from the library's own events and the entry count, beside Fisher's table build, and k_permute_minp / the
step-down kernels over the CMH tables beside the same kernels over Fisher's tables on the same label rows, the
variants alternating inside every repeat (profiles/cmh_wy.txt).
    python tools/cmh_bench.py [repeats] wy"""
import os, sys, time, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from scoary_amd import synth
from scoary_amd.engine import AssociationEngine, pack_bits_rows

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
WY = "wy" in sys.argv[2:]
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


def westfall_young():
    """S11 at this shape: tables and passes, CMH beside Fisher, alternating."""
    med = statistics.median
    res = eng.associate(gm, trv, mkv, permutations=0, plan=plan)
    sd_names = ("k_stepdown_prep", "k_stepdown_minp_cells", "k_stepdown_minp_count", "k_stepdown_sum")

    def timed(names, fn):
        eng.set_timing(True)
        try:
            out = fn()
            return out, [eng.kernel_ms(n) for n in names]
        finally:
            eng.set_timing(False)

    def ranked(values):
        vs, order = torch.sort(values.contiguous(), dim=1, stable=True)
        return vs.contiguous(), order.to(torch.int32).contiguous()

    for name, sp in variants:
        cm = eng.cmh(gm, trv, mkv, sp)
        perms = eng.perm_generate(mkv, res["margins"], N, P, 0, seed, strata=sp)
        build = {"fisher": lambda: eng.minp_tables(res["counts"]), "cmh": lambda: eng.cmh_tables(gm, mkv, sp, cm)}
        events = {"fisher": ("k_minp_plan", "k_minp_fill"), "cmh": ("k_cmh_minp_plan", "k_cmh_minp_fill")}
        tables = {kind: build[kind]() for kind in build}                       # warm-up, and the tables of the passes
        observed = {"fisher": res["p"], "cmh": eng.cmh_observed(tables["cmh"], cm["a"])}
        rank = {kind: ranked(observed[kind]) for kind in build}
        minp = torch.ones((T, P), dtype=torch.float64, device=eng.device)
        c = torch.zeros((T, G), dtype=torch.int32, device=eng.device)
        for kind in build:                                                     # warm-up of both passes
            eng.permute_minp(gm, perms, tables[kind], minp)
            eng.permute_stepdown(gm, perms, tables[kind], rank[kind][1], rank[kind][0], c, minp=minp)
        torch.cuda.synchronize()
        print("%-12s entries: cmh %.1f M (%.1f per pair), fisher %.1f M (%.1f per pair)"
              % (name, tables["cmh"].entries / 1e6, tables["cmh"].entries / (T * G), tables["fisher"].entries / 1e6,
                 tables["fisher"].entries / (T * G)), flush=True)
        plan_ms, fill_ms = {k: [] for k in build}, {k: [] for k in build}
        single, down = {k: [] for k in build}, {k: [] for k in build}
        for i in range(REPEATS):
            for kind in (("fisher", "cmh") if i % 2 == 0 else ("cmh", "fisher")):
                _t, (a, b) = timed(events[kind], build[kind])
                plan_ms[kind].append(a); fill_ms[kind].append(b)
                del _t
                _m, (ms,) = timed(("k_permute_minp",), lambda: eng.permute_minp(gm, perms, tables[kind], minp))
                single[kind].append(ms)
                _c, got = timed(sd_names, lambda: eng.permute_stepdown(gm, perms, tables[kind], rank[kind][1],
                                                                       rank[kind][0], c, minp=minp))
                down[kind].append(sum(got))
        for kind in build:
            print("%-12s %-6s tables: plan median %.3f ms (min %.3f max %.3f)  fill median %.3f ms (min %.3f max %.3f)"
                  % (name, kind, med(plan_ms[kind]), min(plan_ms[kind]), max(plan_ms[kind]), med(fill_ms[kind]),
                     min(fill_ms[kind]), max(fill_ms[kind])), flush=True)
        for kind in build:
            print("%-12s %-6s passes: k_permute_minp median %.3f ms (min %.3f max %.3f)  step-down kernels median "
                  "%.3f ms (min %.3f max %.3f)" % (name, kind, med(single[kind]), min(single[kind]), max(single[kind]),
                                                   med(down[kind]), min(down[kind]), max(down[kind])), flush=True)
        del tables, perms


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


if WY:
    westfall_young()
    sys.exit(0)

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
