"""The launch plan of k_permute_mfma (scoary_mfma_plan, host only): ranges over the linear (trait, stage) sequence.

For each 256-slot gene block the work is Q = T * S stages (S = ceil(P / 64) per trait), cut into R ranges of
L = ceil(Q / R) stages, the last one maybe shorter.  A candidate R is admissible if L <= 1023 (a segment's count
stays within 16 bits) and every trait meets at most ntiles = ceil(P / 512) ranges (each of its segments has a
partial tile of its own).  The library picks the admissible R with the smallest model cost

    ceil(gene_blocks * R / num_cu) * (L + c_start + switches * c_switch),

switches = the most traits any range enters after its first.  The rule is restated here in numpy, sharing no
code with the library; the two constants are read from the source, they are measured and may move.
"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NUM_CU = (8, 256, 304)
K_SPLIT = (256, 33 * 256, 128 * 256, 196 * 256)
TRAITS = (1, 3, 10, 50)
PERMS = (1, 64, 193, 512, 513, 1100, 10000, 65472, 65473, 70000)


@pytest.fixture(scope="module")
def lib():
    from scoary_amd import _abi
    return _abi.load()


@pytest.fixture(scope="module")
def constants():
    src = open(os.path.join(ROOT, "scoary_amd", "csrc", "scoary_mfma.hip")).read()
    c = {}
    for name in ("kMfmaBlockStartStages", "kMfmaTraitSwitchStages"):
        m = re.search(r"const double %s = ([0-9.]+);" % name, src)
        assert m, name
        c[name] = float(m.group(1))
    assert c["kMfmaBlockStartStages"] > 0.0 and c["kMfmaTraitSwitchStages"] >= 0.0
    return c["kMfmaBlockStartStages"], c["kMfmaTraitSwitchStages"]


def plan(lib, num_cu, k_split, T, P):
    out = (ctypes.c_int64 * 4)()
    assert lib.scoary_mfma_plan(num_cu, k_split, T, P, out) == 0
    return tuple(int(v) for v in out)          # gene_blocks, R, L, blocks


def segments_per_trait(T, S, L):
    t = np.arange(T, dtype=np.int64)
    return ((t + 1) * S - 1) // L - t * S // L + 1


def candidates(T, P):
    """Every admissible (R, L, switches): R the smallest count of ranges that gives L."""
    S, ntiles = -(-P // 64), -(-P // 512)
    Q = T * S
    out = []
    R_all = np.arange(1, Q + 1, dtype=np.int64)
    L_all = -(-Q // R_all)
    for L in np.unique(L_all)[::-1].tolist():
        if L > 1023 or segments_per_trait(T, S, L).max() > ntiles:
            continue
        R = int(R_all[L_all == L][0])
        r = np.arange(-(-Q // L), dtype=np.int64)
        switches = int(((np.minimum(Q, (r + 1) * L) - 1) // S - r * L // S).max())
        out.append((R, L, switches))
    return out


def cost(num_cu, gene_blocks, L, switches, Q, c_start, c_switch):
    rounds = -(-gene_blocks * -(-Q // L) // num_cu)
    return float(rounds) * (float(L) + c_start + float(switches) * c_switch)


@pytest.mark.parametrize("T", TRAITS)
@pytest.mark.parametrize("P", PERMS)
def test_plan_invariants_and_cheapest(lib, constants, T, P):
    c_start, c_switch = constants
    S, ntiles = -(-P // 64), -(-P // 512)
    Q = T * S
    cands = candidates(T, P)
    assert cands, "no admissible R at all"
    by_L = {L: sw for _R, L, sw in cands}
    for num_cu in NUM_CU:
        for k_split in K_SPLIT:
            gb, R, L, blocks = plan(lib, num_cu, k_split, T, P)
            what = "num_cu %d k_split %d T %d P %d: R %d L %d" % (num_cu, k_split, T, P, R, L)
            assert gb == -(-k_split // 256) and blocks == gb * R, what
            # the ranges [r L, min((r + 1) L, Q)) tile [0, Q), none of them empty
            assert L == -(-Q // R) and (R - 1) * L < Q <= R * L, what
            assert 1 <= L <= 1023, what
            assert segments_per_trait(T, S, L).max() <= ntiles, what
            # tile index of trait t's segment in range r: r - floor(t S / L), distinct inside the trait, < ntiles
            for t in range(T):
                first, last = t * S // L, ((t + 1) * S - 1) // L
                tiles = [r - first for r in range(first, last + 1)]
                assert len(set(tiles)) == len(tiles) and 0 <= min(tiles) and max(tiles) < ntiles, what
            assert L in by_L, what + ": not a candidate of the rule"
            mine = cost(num_cu, gb, L, by_L[L], Q, c_start, c_switch)
            for _R2, L2, sw2 in cands:
                assert mine <= cost(num_cu, gb, L2, sw2, Q, c_start, c_switch), what + " against L %d" % L2


def test_plan_choices_the_gpu_cases_rest_on(lib):
    """tests/test_gpu_mfma_ranges.py at 256 CUs: (a) three whole traits in one block, (b) two ranges that cut the
    middle trait (T = 3: after its stage 8) or meet three traits each (T = 5)."""
    assert plan(lib, 256, 65536, 3, 193) == (256, 1, 12, 256)
    for P in (1100, 1152):
        assert plan(lib, 256, 32768, 3, P) == (128, 2, 27, 256)
        assert plan(lib, 256, 32768, 5, P) == (128, 2, 45, 256)


def test_plan_refuses_bad_arguments(lib):
    out = (ctypes.c_int64 * 4)()
    for args in ((0, 256, 1, 1), (256, 0, 1, 1), (256, 256, 0, 1), (256, 256, 1, 0)):
        assert lib.scoary_mfma_plan(*args, out) != 0
    assert lib.scoary_mfma_plan(256, 256, 1, 1, None) != 0
