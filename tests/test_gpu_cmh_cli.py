"""--cmh on the command line: the reference's exampledata with --no_pairwise and a strata file -- the CMH columns
come last and hold the engine's values as the writer formats every float; without --cmh the files are the bytes
of the same run on the flags that were there before."""
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
        text = f.read()
    with open([os.path.join(str(outdir), f) for f in os.listdir(str(outdir)) if f.endswith(".log")][0]) as f:
        return text, list(csv.reader(io.StringIO(text))), f.read()


def test_cli_cmh_columns_are_the_engines_values(exampledir, tmp_path):
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
        f.write("Isolate,Lineage\n" + "".join("%s,%s\n" % (s, ("clade A", "clade B", "7")[(i * 7 // N) % 3])
                                               for i, s in enumerate(strains)))
    base = ["-g", os.path.join(exampledir, "Gene_presence_absence.csv"),
            "-t", os.path.join(exampledir, "Tetracycline_resistance.csv"), "--no_pairwise", "--seed", str(CLI_SEED),
            "-p", "1.0"]
    perm = base + ["-e", str(P)]
    plain_text, plain, _ = run_cli(base, tmp_path / "plain")
    strat_text, strat, _ = run_cli(perm + ["--permute-strata", three], tmp_path / "strata")
    _t, no_perm, log = run_cli(base + ["--cmh", three], tmp_path / "cmh")
    _t, with_perm, log_perm = run_cli(perm + ["--cmh", three], tmp_path / "cmh_perm")
    _t, both, _ = run_cli(perm + ["--cmh", three, "--permute-strata", three], tmp_path / "both")
    assert "Cochran-Mantel-Haenszel test over 3 strata" in log and "Permuting trait labels" not in log
    assert "Permuting trait labels within 3 strata" in log_perm
    # the columns come last; everything in front of them is the file of the run without --cmh, cell for cell
    assert no_perm[0] == plain[0] + ["CMH_p", "CMH_odds_ratio"]
    assert with_perm[0] == strat[0] + ["CMH_p", "CMH_odds_ratio", "CMH_empirical_p"] and strat[0][-1] == "Empirical_p"
    assert [r[:-2] for r in no_perm] == plain and [r[:-3] for r in with_perm] == strat and both == with_perm
    assert len(plain) > 10
    # the engine, called directly with the same seed and strata
    eng = m.get_engine()
    idx, _labels = m.strata_indices(m.read_strata_file(three), strains)
    trv = eng.vecrows(pack_bits_rows((traits == 1).astype(np.uint8)), N)
    mkv = eng.vecrows(pack_bits_rows((traits != 2).astype(np.uint8)), N)
    sp = eng.strata_plan(idx, trv, mkv, N)
    res = eng.associate(eng.pack_dense(genes), trv, mkv, permutations=P, seed=CLI_SEED, strata=sp, cmh=True)
    p, odds = res["cmh_p"].cpu().numpy()[0], res["cmh_odds"].cpu().numpy()[0]
    r = res["r_cmh"].cpu().numpy().view(np.uint32)[0]
    for rows in (no_perm, with_perm):
        for d in rows[1:]:
            g = ids.index(d[0])
            cells = d[len(plain[0]) + (1 if rows is with_perm else 0):]
            assert cells[0] == repr(float(p[g])) and cells[1] == repr(float(odds[g])), d[0]
            if rows is with_perm:
                assert cells[2] == repr((float(r[g]) + 1.0) / (P + 1.0)), d[0]
    assert len({d[-1] for d in with_perm[1:]}) > 3
    # without --cmh: the bytes of the same runs as the parent's flag set writes them (no CMH column, nothing else moved)
    again_text, _rows, _ = run_cli(base, tmp_path / "plain_again")
    assert again_text == plain_text and "CMH" not in plain_text and "CMH" not in strat_text
    # (that those bytes are the reference's is test_gpu_cli.py's business: the same arguments, against tests/golden)
    gold = list(csv.reader(io.StringIO(golden_text("csv_no_pairwise/Tetracycline_resistance.results.csv.gz"))))
    assert plain[0] == gold[0] and sorted(r[:7] for r in plain) == sorted(r[:7] for r in gold)
