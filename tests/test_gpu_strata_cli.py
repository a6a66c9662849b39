"""--permute-strata on the command line: the reference's exampledata with --no_pairwise -e 200 --permute-fwer and a
strata file -- only Empirical_p and Westfall_Young_p change, and they are the engine's (r + 1) / (P + 1)."""
import csv
import io
import os
import sys

import numpy as np
import pytest

from conftest import golden_text, read_dense

pytestmark = pytest.mark.gpu
P, CLI_SEED = 200, 4321


def run_cli(argv, outdir):
    from scoary_amd import methods as m
    old = sys.argv
    sys.argv = ["scoary"] + argv + ["-o", str(outdir), "--no-time"]
    try:
        with pytest.raises(SystemExit) as e:
            m.main()
        assert e.value.code in (0, None), e.value.code
    finally:
        sys.argv = old
    with open(os.path.join(str(outdir), "Tetracycline_resistance.results.csv"), newline="") as f:
        rows = list(csv.reader(io.StringIO(f.read())))
    with open([os.path.join(str(outdir), f) for f in os.listdir(str(outdir)) if f.endswith(".log")][0]) as f:
        return rows, f.read()


def _argv(exampledir):
    return ["-g", os.path.join(exampledir, "Gene_presence_absence.csv"),
            "-t", os.path.join(exampledir, "Tetracycline_resistance.csv"),
            "--no_pairwise", "-e", str(P), "--permute-fwer", "--seed", str(CLI_SEED), "-p", "1.0"]


def test_cli_strata_change_only_the_permutation_columns(exampledir, tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from scoary_amd import methods as m
    from scoary_amd.engine import pack_bits_rows
    ids, strains, genes, names, traits = read_dense(golden_text("exampledata/Gene_presence_absence.csv.gz"),
                                                    golden_text("exampledata/Tetracycline_resistance.csv.gz"))
    N = len(strains)
    three = os.path.join(str(tmp_path), "three.csv")
    with open(three, "w") as f:
        f.write("Isolate,Lineage,Comment\nnot_in_the_table,L9,\n")
        for i, s in reversed(list(enumerate(strains))):
            f.write("%s,%s,whatever\n" % (s, ("clade A", "clade B", "7")[(i * 7 // N) % 3]))
    own = os.path.join(str(tmp_path), "own.csv")
    with open(own, "w") as f:
        f.write("Isolate,Stratum\n" + "".join("%s,s%d\n" % (s, i) for i, s in enumerate(strains)))
    plain, _ = run_cli(_argv(exampledir), tmp_path / "plain")
    strat, log = run_cli(_argv(exampledir) + ["--permute-strata", three], tmp_path / "three")
    head = plain[0]
    assert strat[0] == head and len(strat) == len(plain) > 10
    ce, cw = head.index("Empirical_p"), head.index("Westfall_Young_p")
    keep = [c for c in range(len(head)) if c not in (ce, cw)]
    assert [[r[c] for c in keep] for r in strat] == [[r[c] for c in keep] for r in plain]
    assert [r[ce] for r in strat] != [r[ce] for r in plain]
    sizes = np.bincount([(i * 7 // N) % 3 for i in range(N)])
    assert "within 3 strata of %d to %d isolates" % (sizes.min(), sizes.max()) in log
    # the engine, called directly with the same seed and strata
    eng = m.get_engine()
    idx, labels = m.strata_indices(m.read_strata_file(three), strains)
    assert labels == ["clade A", "clade B", "7"]
    trv = eng.vecrows(pack_bits_rows((traits == 1).astype(np.uint8)), N)
    mkv = eng.vecrows(pack_bits_rows((traits != 2).astype(np.uint8)), N)
    sp = eng.strata_plan(idx, trv, mkv, N)
    res = eng.associate(eng.pack_dense(genes), trv, mkv, permutations=P, seed=CLI_SEED, strata=sp, fwer=True)
    r = res["r"].cpu().numpy().view(np.uint32)[0]
    rf = res["r_fwer"].cpu().numpy()[0]
    for d in strat[1:]:
        g = ids.index(d[0])
        assert d[ce] == repr((float(r[g]) + 1.0) / (P + 1.0)), d[0]
        assert d[cw] == repr((float(rf[g]) + 1.0) / (P + 1.0)), d[0]
    # every isolate its own stratum: no labelling but the observed one
    alone, log = run_cli(_argv(exampledir) + ["--permute-strata", own], tmp_path / "own")
    assert "within %d strata of 1 to 1 isolates" % N in log
    assert all(d[ce] == "1.0" and d[cw] == "1.0" for d in alone[1:]) and len(alone) == len(plain)
