"""The step-down maxT passes over the statistics of the categorical traits (spec S23) next to the single-step kernels and
the count kernels they restate, at cfg3's geometry with ten categorical traits on one MI355X: G = 50 000 genes, N = 2000
isolates (or the first ``isolates`` of them), T = 10, P = 10 000 label permutations, K = 4 and K = 8 classes, 10 strata
for the generalized CMH test.

Timed, every repeat in the same process, the variants alternating inside a repeat (their order reversed in every
other repeat):
  * k_cat_permute and k_cat_maxt (the yardsticks), k_cat_sd_max, k_cat_sd_suffix and k_cat_sd_count (one call of
    scoary_permute_cat_stepdown) and k_cat_sd_gather by device events (set_timing / kernel_ms), each launched through
    its raw entry point over ONE set of code rows, generated once; the same for the generalized CMH kernels over rows
    shuffled within the strata;
  * the whole permutation step by a host clock around a device synchronise: the engine's step without a family-wise
    flag, with --categorical-fwer and with --categorical-fwer-stepdown (the sort, the gather, the row generator, the
    three launches, the tail and the single-step search).
Before anything is timed the step-down passes are held to the other two kernels (r by rank position against the count
kernel's d_r, maxs against the single-step kernel's, all of both) and to the statistic computed in fp64 tensor
operations -- each rounded once, in the spec's order -- over the first 256 permutations of trait 0 (c of every rank).
Reported: median, min and max of each, and the two passes together against the single-step kernel: the counts are formed
twice, so about 2 x is what the design predicts.  Raw lines on stdout (profiles/cat_stepdown.txt).
    python tools/bench_cat_stepdown.py [repeats] [warmup] [isolates]"""
import datetime
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from scoary_amd import synth
from scoary_amd.engine import AssociationEngine

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 2
T, CHECK_P, STRATA = 10, 256, 10
SHARES = {4: [0.4, 0.3, 0.2, 0.1], 8: [0.3, 0.2, 0.15, 0.1, 0.1, 0.05, 0.05, 0.05]}

if not torch.cuda.is_available():
    sys.exit("bench_cat_stepdown needs an MI355X: there is nothing to time without one")
genes, _traits, P, seed = synth.make_config("cfg3", T=1)
if len(sys.argv) > 3:
    genes = np.ascontiguousarray(genes[:, :int(sys.argv[3])])
G, N = genes.shape
eng = AssociationEngine(0)
gm = eng.pack_dense(genes)
dense = torch.from_numpy(genes).to(eng.device).to(torch.float64)
print("date %s  shape G=%d N=%d T=%d P=%d S=%d  repeats %d warm-up %d" % (
    datetime.date.today().isoformat(), G, N, T, P, STRATA, REPEATS, WARMUP), flush=True)


def sync_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def kernel(fn, *names):
    eng.set_timing(True)
    try:
        fn()
        torch.cuda.synchronize()
        return [eng.kernel_ms(name) for name in names]
    finally:
        eng.set_timing(False)


def zeros(dtype=torch.int32, shape=None):
    return torch.zeros(shape or (T, G), dtype=dtype, device=eng.device)


def tables(rows):
    """a float64 [P', G, 7] of the dense genes against code rows [P', N]: exact integer products."""
    return torch.stack([dense @ (rows == k + 1).to(torch.float64).t() for k in range(7)], dim=-1).permute(1, 0, 2)


def chi2_cells(rows, a_obs, nk, inv, ivm):
    """S22's chi-square statistic of trait 0 under rows [P', N]: float64 [P', G], the spec's operations in its order."""
    a7 = tables(rows)
    m = a_obs.sum(dim=1).to(torch.float64)                                    # [G]
    n = float(nk.sum())
    klast = int(torch.nonzero(nk).max()) + 1
    tot, used = torch.zeros(a7.shape[:2], dtype=torch.float64, device=eng.device), 0.0
    for k in range(klast):
        a = a7[..., k] if k < klast - 1 else m[None, :] - used
        used = used + a if k < klast - 1 else used
        c = n * a - m[None, :] * float(nk[k])
        tot = tot + (c * c) * inv[k]
    return tot * ivm[None, :]


def gcmh_cells(rows, form):
    """Q of trait 0 under rows [P', N] and the forms [G, 35]: float64 [P', G]."""
    a7 = tables(rows)
    y, f0 = [], 7
    for i in range(7):
        x = a7[..., i] - form[None, :, i]
        for j in range(i):
            x = x - form[None, :, f0 + i * (i - 1) // 2 + j] * y[j]
        y.append(x)
    q = torch.zeros(a7.shape[:2], dtype=torch.float64, device=eng.device)
    for j in range(7):
        q = q + (y[j] * y[j]) * form[None, :, 28 + j]
    return q


def held_to(cells, thr0, order0, c0, what):
    s = cells.t()[order0]
    u = torch.flip(torch.cummax(torch.flip(s, dims=(0,)), dim=0).values, dims=(0,)).clamp_(min=0.0)
    want = (u >= thr0[order0][:, None]).sum(dim=1).to(torch.int32)
    bad = int((want != c0).sum())
    print("%s: c of trait 0 over %d permutations against the fp64 tensor route: %d of %d ranks differ" % (
        what, CHECK_P, bad, G), flush=True)
    return bad


for K in (4, 8):
    rng = np.random.default_rng(seed + 23 + K)
    codes = np.stack([rng.choice(np.arange(1, K + 1), size=N, p=SHARES[K]) for _ in range(T)])
    codes[rng.random((T, N)) < 0.01] = 0
    strata = rng.integers(0, STRATA, N)
    strata[0] = STRATA - 1
    cplan, gplan = eng.categorical_plan(codes), eng.gcmh_plan(codes, strata)
    cobs, gobs = eng.categorical(gm, cplan), eng.gcmh(gm, gplan)
    inv, ivm, _sobs, cthr = eng.categorical_wy_prepare(cplan, cobs["a"])
    sides = {}
    for name, plan, thr, rows in (("cat", cplan, cthr, eng.categorical_rows(cplan, 0, P, seed)),
                                  ("gcmh", gplan, gobs["thr"], eng.gcmh_rows(gplan, 0, P, seed))):
        order32, tt = eng.rank_stepdown_order(thr)
        if name == "cat":
            scratch = eng.cat_stepdown_gather(gm, order32, cobs["a"], ivm, thr, N, P)
        else:
            scratch = eng.gcmh_stepdown_gather(gm, order32, gobs["form"], thr, N, P)
        sides[name] = dict(plan=plan, thr=thr, rows=rows, order32=order32, tt=tt, scratch=scratch, r_count=zeros(),
                           r_maxt=zeros(), r_rank=zeros(), c_rank=zeros(), maxs=zeros(torch.float64, (T, P)),
                           maxs_sd=zeros(torch.float64, (T, P)))
        print("K=%d %s: scratch %.1f MB (gmax %.1f MB), code rows %.1f MB" % (
            K, name, scratch.numel() / 1e6, 8e-6 * T * (-(-G // 1024) * 16) * (-(-P // 64) * 64),
            rows.numel() * 2 / 1e6), flush=True)

    def count_pass(name):
        s = sides[name]
        s["r_count"].zero_()
        if name == "cat":
            eng.permute_categorical(gm, cplan, cobs["a"], s["rows"], s["r_count"])
        else:
            eng.permute_gcmh(gm, gplan, gobs, s["rows"], s["r_count"])

    def maxt_pass(name):
        s = sides[name]
        s["r_maxt"].zero_()
        s["maxs"].zero_()
        if name == "cat":
            eng.permute_categorical(gm, cplan, cobs["a"], s["rows"], s["r_maxt"], maxt=(inv, ivm, s["maxs"]))
        else:
            eng.permute_gcmh(gm, gplan, gobs, s["rows"], s["r_maxt"], maxt=s["maxs"])

    def sd_passes(name, rows=None, c_rank=None):
        s = sides[name]
        rows = s["rows"] if rows is None else rows
        c_rank = s["c_rank"] if c_rank is None else c_rank
        s["r_rank"].zero_()
        c_rank.zero_()
        if name == "cat":
            eng.permute_cat_stepdown(s["scratch"], cplan, inv, rows, G, 0, s["r_rank"], c_rank, s["maxs_sd"])
        else:
            eng.permute_gcmh_stepdown(s["scratch"], gplan, rows, G, 0, s["r_rank"], c_rank, s["maxs_sd"])

    def gather_pass(name):
        s = sides[name]
        if name == "cat":
            eng._check(eng.lib.scoary_cat_stepdown_gather(
                eng.h, eng._ptr(gm.tiled), eng._ptr(s["order32"]), eng._ptr(cobs["a"]), eng._ptr(ivm),
                eng._ptr(s["thr"]), G, T, N, eng._ptr(s["scratch"]), eng._stream()), "scoary_cat_stepdown_gather")
        else:
            eng._check(eng.lib.scoary_gcmh_stepdown_gather(
                eng.h, eng._ptr(gm.tiled), eng._ptr(s["order32"]), eng._ptr(gobs["form"]), eng._ptr(s["thr"]), G, T, N,
                eng._ptr(s["scratch"]), eng._stream()), "scoary_gcmh_stepdown_gather")

    # -- the checks: nothing is timed that computes something else
    for name in ("cat", "gcmh"):
        s = sides[name]
        count_pass(name)
        maxt_pass(name)
        sd_passes(name)
        torch.cuda.synchronize()
        bad_r = int((s["r_rank"] != s["r_count"].gather(1, s["order32"].to(torch.int64))).sum())
        bad_m = int((s["maxs_sd"].view(torch.int64) != s["maxs"].view(torch.int64)).sum())
        print("K=%d %s: r by rank against the count kernel: %d of %d cells differ; maxs against the single-step "
              "kernel: %d of %d differ" % (K, name, bad_r, T * G, bad_m, T * P), flush=True)
        c_chk = zeros()
        head = s["rows"][:, :CHECK_P].contiguous()
        sd_passes(name, head, c_chk)
        o0 = s["order32"][0].to(torch.int64)
        if name == "cat":
            cells = chi2_cells(head[0], cobs["a"][0], cplan.nk[0], inv[0], ivm[0])
        else:
            cells = gcmh_cells(head[0], gobs["form"][0])
        bad_c = held_to(cells, s["thr"][0], o0, c_chk[0], "K=%d %s" % (K, name))
        del cells
        if bad_r or bad_m or bad_c:
            sys.exit("the step-down passes disagree: nothing is timed")
        sd_passes(name)                                                       # (maxs_sd back to all P columns)
    steps = {
        "cat": (lambda: eng.categorical_permute(gm, cplan, cobs["a"], P, seed),
                lambda: eng.categorical_westfall_young(gm, cplan, cobs, P, seed),
                lambda: eng.categorical_stepdown(gm, cplan, cobs, P, seed)),
        "gcmh": (lambda: eng.gcmh_permute(gm, gplan, gobs, P, seed),
                 lambda: eng.gcmh_westfall_young(gm, gplan, gobs, P, seed),
                 lambda: eng.gcmh_stepdown(gm, gplan, gobs, P, seed)),
    }
    for name, (_plain, _fwer, stepdown) in steps.items():
        r, r_fwer, r_sd, mx = stepdown()
        if not (torch.equal(r, sides[name]["r_count"]) and torch.equal(mx, sides[name]["maxs"])):
            sys.exit("the engine's step disagrees with the raw entry points: nothing is timed")
        print("K=%d %s: r <= r_sd in %d, r_sd <= r_fwer in %d, r_sd < r_fwer in %d of %d cells" % (
            K, name, int((r <= r_sd).sum()), int((r_sd <= r_fwer).sum()), int((r_sd < r_fwer).sum()), T * G), flush=True)
        del r, r_fwer, r_sd, mx

    KERNELS = {"cat": ("k_cat_permute", "k_cat_maxt", ("k_cat_sd_max", "k_cat_sd_suffix", "k_cat_sd_count")),
               "gcmh": ("k_gcmh_permute", "k_gcmh_maxt", ("k_gcmh_sd_max", "k_cat_sd_suffix", "k_gcmh_sd_count"))}
    variants = {}
    for name in ("cat", "gcmh"):
        pk, mk, sdk = KERNELS[name]
        variants[(name, pk)] = lambda name=name, pk=pk: kernel(lambda: count_pass(name), pk)
        variants[(name, mk)] = lambda name=name, mk=mk: kernel(lambda: maxt_pass(name), mk)
        variants[(name,) + sdk] = lambda name=name, sdk=sdk: kernel(lambda: sd_passes(name), *sdk)
        variants[(name, "k_cat_sd_gather")] = lambda name=name: kernel(lambda: gather_pass(name), "k_cat_sd_gather")
        for label, fn in zip(("step, no family-wise flag", "step, --categorical-fwer",
                              "step, --categorical-fwer-stepdown"), steps[name]):
            variants[(name, label)] = lambda fn=fn: [sync_ms(fn)[1]]
    t = {}
    for i in range(WARMUP + REPEATS):
        order = list(variants)
        for key in (order if i % 2 == 0 else order[::-1]):
            ms = variants[key]()
            if i >= WARMUP:
                for kname, x in zip(key[1:], ms):
                    t.setdefault((key[0], kname), []).append(x)
    med = {key: statistics.median(xs) for key, xs in t.items()}
    for key, xs in t.items():
        print("K=%d %-5s %-36s median %9.3f ms  min %9.3f  max %9.3f  (n=%d)" % (
            K, key[0], key[1], med[key], min(xs), max(xs), len(xs)), flush=True)
        print("raw N=%d K=%d %s %s %s" % (N, K, key[0], key[1].replace(" ", "_"), " ".join("%.4f" % x for x in xs)),
              flush=True)
    for name in ("cat", "gcmh"):
        pk, mk, (ak, sk, bk) = KERNELS[name]
        a, b, sfx, one = med[(name, ak)], med[(name, bk)], med[(name, sk)], med[(name, mk)]
        xs = t[(name, mk)]
        print("K=%d: %s / %s = %.3f; %s / %s = %.3f; both passes / %s = %.3f (the design predicts about 2); with the "
              "suffix walk %.3f; %s's spread %.3f ms, %.1f %% of its median" % (
                  K, ak, mk, a / one, bk, mk, b / one, mk, (a + b) / one, (a + b + sfx) / one, mk, max(xs) - min(xs),
                  100.0 * (max(xs) - min(xs)) / one), flush=True)
        sd_ms, fw_ms, no_ms = (med[(name, label)] for label in ("step, --categorical-fwer-stepdown",
                                                                "step, --categorical-fwer",
                                                                "step, no family-wise flag"))
        print("K=%d %s: step with --categorical-fwer-stepdown / with --categorical-fwer = %.3f; / without either = %.3f"
              % (K, name, sd_ms / fw_ms, sd_ms / no_ms), flush=True)
    del sides
try:
    import __graft_entry__ as ge
    with open(ge.HIP_RESOURCES) as f:
        res = json.load(f)
    for kname, fields in sorted(res.items()):
        if any(k in kname for k in ("k_cat_permute", "k_cat_maxt", "k_gcmh_permute", "k_gcmh_maxt", "k_cat_sd_",
                                    "k_gcmh_sd_")):
            print("%s resources: " % kname + ", ".join("%s %s" % kv for kv in sorted(fields.items())), flush=True)
except (OSError, ImportError, ValueError):
    print("kernel resources: the build's report was not found", flush=True)
try:            # clocks and power: read, never set
    smi = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=30)
    lines = [ln.strip() for ln in smi.stdout.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "Power" in ln)]
    print("telemetry after the run (rocm-smi, GPU 0): " + ("; ".join(lines) if lines else "not read"), flush=True)
except (OSError, subprocess.SubprocessError):
    print("telemetry: clocks and power not read", flush=True)
