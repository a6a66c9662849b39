"""Per-kernel times of the permutation step under the three routing modes of the matrix-core kernel
(none / all / auto), on a BASELINE config's shape: what k_permute_mfma costs next to k_permute_lists on the same
genes, and the two rates the break-even constants of scoary_mfma.hip (kMfmaNsPerGene, kListNsPerEntry) are derived
from.  The step is the engine's: the label generator writes the B fragments itself (k_mfma_bfrag does not run and
counts as 0; the generator's time is listed beside it); --unfused puts the conversion pass back (tiles from
elsewhere).  r is compared with the dense kernel.

    python tools/mfma_route_bench.py [--config cfg3] [--gene-kind balanced] [--steps 5] [--unfused] [--sweep P,P,...]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from scoary_amd import synth
    from scoary_amd.engine import AssociationEngine, pack_bits_rows
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--gene-kind", default=None)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--sweep", default=None, metavar="P,P,...",
                    help="also time k_permute_mfma with every gene routed at these permutation counts and fit "
                         "the plan's constants (e.g. 512,1024,2048,3072,4096,6144,8192,10000)")
    ap.add_argument("--unfused", action="store_true",
                    help="generate the tiles alone and convert them with k_mfma_bfrag (engine.fuse_bfrag = False)")
    args = ap.parse_args()
    genes, traits, P, seed = synth.make_config(args.config, gene_kind=args.gene_kind)
    G, N = genes.shape
    T = traits.shape[0]
    eng = AssociationEngine(0)
    eng.fuse_bfrag = not args.unfused
    gm = eng.pack_dense(genes)
    eng.build_lists(gm)
    L = gm.lists
    tb = pack_bits_rows((traits == 1).astype(np.uint8))
    mb = pack_bits_rows((traits != 2).astype(np.uint8))
    trv, mkv = eng.vecrows(tb, N), eng.vecrows(mb, N)
    want = eng.associate(gm, trv, mkv, permutations=P, seed=seed, use_lists=False)["r"].cpu().numpy().copy()
    ws = eng.workspace(gm, T, P, use_lists=True)
    padded = int(L.block_start[-1])
    out = {"config": args.config, "gene_kind": args.gene_kind or "config", "G": G, "N": N, "T": T, "P": P,
           "padded_entries": padded, "fused_bfrag": eng.fuse_bfrag,
           "breakeven_entries": int(eng.lib.scoary_mfma_breakeven_entries()), "modes": {}}
    names = ("k_permute_lists", "k_permute_mfma", "k_mfma_bfrag", "k_lists_reduce", "k_perm_generate_tiles")
    for mode in ("none", "all", "auto"):
        eng.set_mfma_route(mode)
        k_split = eng.mfma_split(gm, T, P)
        routed = int(L.block_start[-1 if k_split >= G else k_split // 256]) if k_split else 0
        for _ in range(2):
            res = eng.associate(gm, trv, mkv, permutations=P, seed=seed, use_lists=True, workspace=ws, graph=False)
        torch.cuda.synchronize()
        ok = bool(np.array_equal(res["r"].cpu().numpy(), want))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            eng.associate(gm, trv, mkv, permutations=P, seed=seed, use_lists=True, workspace=ws, graph=False)
        e1.record()
        torch.cuda.synchronize()
        step_ms = e0.elapsed_time(e1) / args.steps
        eng.set_timing(True)
        ms = {n: [] for n in names}
        for _ in range(3):
            eng.associate(gm, trv, mkv, permutations=P, seed=seed, use_lists=True, workspace=ws, graph=False)
            torch.cuda.synchronize()
            for n in names:
                try:
                    ms[n].append(eng.kernel_ms(n))
                except Exception:
                    ms[n].append(0.0)
        eng.set_timing(False)
        med = {n: float(np.median(v)) for n, v in ms.items()}
        row = {"k_split": k_split, "routed_entries": routed, "r_equals_dense": ok, "step_ms": step_ms,
               "kernel_ms": med}
        scale = 1e5 / (T * P)              # per 100 000 tests of a gene
        if k_split:
            row["mfma_ns_per_gene"] = (med["k_permute_mfma"] + med["k_mfma_bfrag"]) * 1e6 / k_split * scale
            row["mfma_mac_per_s"] = k_split * 2048.0 * T * P / (med["k_permute_mfma"] * 1e-3)
        if padded - routed:
            row["list_ns_per_entry"] = med["k_permute_lists"] * 1e6 / (padded - routed) * scale
        out["modes"][mode] = row
        print(mode, json.dumps(row), flush=True)
    if args.sweep:
        out["sweep"] = sweep(eng, gm, trv, mkv, T, seed, [int(p) for p in args.sweep.split(",")])
    eng.set_mfma_route("auto")
    print(json.dumps(out))


def sweep(eng, gm, trv, mkv, T, seed, perms):
    """k_permute_mfma with every gene routed over a range of P: its launch plan (scoary_mfma_plan), its time, and
    the least-squares fit of  time = rounds x (L + c_start + switches x c_switch) x tau  -- the constants
    kMfmaBlockStartStages and kMfmaTraitSwitchStages of scoary_mfma.hip and the time of a stage."""
    import ctypes

    import torch
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    eng.set_mfma_route("all")
    rows = []
    # the first Tk traits as well: plans of one trait count tend to share their switches, which the fit cannot
    # tell from the start of a block then
    for Tk, P in [(Tk, P) for Tk in sorted({T, max(1, T // 2), min(T, 2), 1}, reverse=True) for P in perms]:
        plan = (ctypes.c_int64 * 4)()
        assert eng.lib.scoary_mfma_plan(num_cu, gm.G, Tk, P, plan) == 0
        gene_blocks, R, L, blocks = (int(v) for v in plan)
        S = -(-P // 64)
        Q = Tk * S
        switches = max((min(Q, (r + 1) * L) - 1) // S - r * L // S for r in range(R))
        tr, mk = trv[:Tk].contiguous(), mkv[:Tk].contiguous()
        ws = eng.workspace(gm, Tk, P, use_lists=True)
        for _ in range(2):
            eng.associate(gm, tr, mk, permutations=P, seed=seed, use_lists=True, workspace=ws, graph=False)
        torch.cuda.synchronize()
        eng.set_timing(True)
        ms = []
        for _ in range(5):
            eng.associate(gm, tr, mk, permutations=P, seed=seed, use_lists=True, workspace=ws, graph=False)
            torch.cuda.synchronize()
            ms.append(eng.kernel_ms("k_permute_mfma"))
        eng.set_timing(False)
        row = {"T": Tk, "P": P, "R": R, "L": L, "blocks": blocks, "rounds": -(-blocks // num_cu),
               "switches": switches, "k_permute_mfma_ms": float(np.median(ms))}
        rows.append(row)
        print("sweep", json.dumps(row), flush=True)
    A = np.array([[r["rounds"] * r["L"], r["rounds"], r["rounds"] * r["switches"]] for r in rows], dtype=np.float64)
    y = np.array([r["k_permute_mfma_ms"] for r in rows])
    if np.linalg.matrix_rank(A) < 3:           # the plans' switches do not vary on their own: two unknowns
        A = A[:, :2]
    coef = np.linalg.lstsq(A, y, rcond=None)[0]
    fit = {"tau_ms_per_stage": float(coef[0]), "c_start_stages": float(coef[1] / coef[0]),
           "c_switch_stages": float(coef[2] / coef[0]) if len(coef) > 2 else None,
           "max_rel_residual": float(np.max(np.abs(A @ coef - y) / y))}
    print("fit", json.dumps(fit), flush=True)
    return {"rows": rows, "fit": fit}


if __name__ == "__main__":
    main()
