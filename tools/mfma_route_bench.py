"""Per-kernel times of the permutation step under the three routing modes of the matrix-core kernel
(none / all / auto), on a BASELINE config's shape: what k_permute_mfma and its B-operand conversion cost
next to k_permute_lists on the same genes, and the two rates the break-even constants of
scoary_mfma.hip (kMfmaNsPerGene, kListNsPerEntry) are derived from.  r is compared with the dense kernel.

    python tools/mfma_route_bench.py [--config cfg3] [--gene-kind balanced] [--steps 5]
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
    args = ap.parse_args()
    genes, traits, P, seed = synth.make_config(args.config, gene_kind=args.gene_kind)
    G, N = genes.shape
    T = traits.shape[0]
    eng = AssociationEngine(0)
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
           "padded_entries": padded,
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
    eng.set_mfma_route("auto")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
