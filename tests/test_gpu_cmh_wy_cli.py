"""--cmh-fwer / --cmh-fwer-stepdown on the command line: the reference's exampledata with --no_pairwise, a
three-stratum file and --permute -- the two columns come after CMH_empirical_p and hold (r + 1) / (P + 1) of the
engine's counts; every other cell is that of the run without the new flags, and --permute-fwer beside them changes
nothing in them."""
import os

import numpy as np
import pytest

from conftest import golden_text, read_dense
from test_gpu_cmh_cli import run_cli

pytestmark = pytest.mark.gpu
P, CLI_SEED = 50, 4321
NEW = ["CMH_Westfall_Young_p", "CMH_Westfall_Young_stepdown_p"]


def test_cli_cmh_westfall_young_columns(exampledir, tmp_path):
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
            "-p", "1.0", "--cmh", three, "--permute", str(P)]
    old_text, old, _ = run_cli(base, tmp_path / "old")
    _t, new, log = run_cli(base + ["--cmh-fwer", "--cmh-fwer-stepdown"], tmp_path / "new")
    _t, single, _ = run_cli(base + ["--cmh-fwer"], tmp_path / "single")
    _t, down, _ = run_cli(base + ["--cmh-fwer-stepdown"], tmp_path / "down")
    _t, four, _ = run_cli(base + ["--cmh-fwer", "--cmh-fwer-stepdown", "--permute-fwer", "--permute-fwer-stepdown"],
                          tmp_path / "four")
    old_fwer_text, old_fwer, _ = run_cli(base + ["--permute-fwer"], tmp_path / "old_fwer")
    assert "Westfall-Young minP of the CMH statistic" in log
    # the two columns follow CMH_empirical_p, which was the last; everything in front is the old file, cell for cell
    assert old[0][-1] == "CMH_empirical_p" and new[0] == old[0] + NEW
    assert [r[:-2] for r in new] == old and len(old) > 10
    assert single[0] == old[0] + NEW[:1] and down[0] == old[0] + NEW[1:]
    assert [r[:-1] for r in single] == old and [r[:-1] for r in down] == old
    assert [r[-1] for r in single] == [r[-2] for r in new] and [r[-1] for r in down] == [r[-1] for r in new]
    # all four Westfall-Young flags: the Fisher columns in their places, the CMH columns unchanged
    at = four[0].index("Westfall_Young_p")
    assert four[0][at:at + 2] == ["Westfall_Young_p", "Westfall_Young_stepdown_p"] and four[0][-2:] == NEW
    assert [r[-2:] for r in four] == [r[-2:] for r in new]
    assert [r[:at] + r[at + 2:] for r in four] == new
    assert [r[:at + 1] + r[at + 2:-2] for r in four] == old_fwer          # --cmh F --permute-fwer: Fisher minima, as before
    # the engine, called directly with the same seed and strata
    eng = m.get_engine()
    idx, _labels = m.strata_indices(m.read_strata_file(three), strains)
    trv = eng.vecrows(pack_bits_rows((traits == 1).astype(np.uint8)), N)
    mkv = eng.vecrows(pack_bits_rows((traits != 2).astype(np.uint8)), N)
    sp = eng.strata_plan(idx, trv, mkv, N)
    res = eng.associate(eng.pack_dense(genes), trv, mkv, permutations=P, seed=CLI_SEED, strata=sp, cmh=True,
                        cmh_fwer=True, cmh_stepdown=True)
    r = res["r_cmh_fwer"].cpu().numpy().view(np.uint32)[0]
    r_sd = res["r_cmh_fwer_sd"].cpu().numpy().view(np.uint32)[0]
    for d in new[1:]:
        g = ids.index(d[0])
        assert d[-2] == repr((float(r[g]) + 1.0) / (P + 1.0)) and d[-1] == repr((float(r_sd[g]) + 1.0) / (P + 1.0)), d[0]
    assert len({d[-2] for d in new[1:]}) > 3 and (r_sd <= r).all()
    # without the new flags: the bytes of the same run
    again_text, _rows, _ = run_cli(base, tmp_path / "old_again")
    assert again_text == old_text and "CMH_Westfall" not in old_text and "CMH_Westfall" not in old_fwer_text
