"""The time stagger of k_permute_mfma at the sizes where the schedule can go wrong.

Wavefronts 4..7 of a block take the block's barrier in the middle of their half stage (behind fragment 15 of
32) and cross their own half boundary -- region test, end of a segment, the next trait's thresholds, LDS-DMA
issue -- without one; wavefronts 0..3 take it in front of a half.  Every slot is routed to the matrix cores and
r is compared bit for bit with the dense AND+popcount kernel on every (gene, trait) pair:

  ticks     T = 1, P = 1, 63, 64: a range of one stage, the late wavefronts' first interval (fragments 0..15
            of half 0) next to their last (the tail behind the final barrier); P = 65, 128, 129, 193: two to
            four stages, the ragged stage first or second of a pair
  switches  T = 3 and T = 5, two traits with missing values.  Each case reads the ranges its launch has from
            scoary_mfma_plan with the device's CU count and asserts the situations it is there for:
              inside         a range begins inside a trait and ends inside a trait
              last_is_first  a trait's last stage is a range's first stage
              last_is_last   a trait's last stage is the last stage of a range that is not the launch's last
              two_switches   a range enters two traits after its first (T = 3: at S = 1, where every stage is
                             its trait's last, and at S = 2 behind a ragged stage)
  slots     G = 33, 129, 160 (one late wavefront owns slots), 256, 257
  K         N = 64, 129, 2000, 2048
  timing    one launch five times, one r
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.set_mfma_route("auto")
    e.close()


@pytest.fixture(scope="module")
def cache():
    """Problems and dense results shared by the tests of this module (built once, never changed)."""
    c = {}
    yield c
    c.clear()


class Problem:
    pass


def _problem(eng, cache, G, N, T, seed=31):
    """Genes over the whole frequency range, an absent and a core gene; traits 1 and 2 have missing values, in
    different places."""
    key = (G, N, T)
    if key in cache:
        return cache[key]
    from scoary_amd.engine import pack_bits_rows
    rng = np.random.default_rng(seed)
    p = Problem()
    p.G, p.N, p.T = G, N, T
    genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    genes[3] = 0
    genes[4] = 1
    traits = (rng.random((T, N)) < 0.4).astype(np.uint8)
    if T > 1:
        traits[1, ::29] = 2
    if T > 2:
        traits[2, 5::17] = 2
    tb = pack_bits_rows((traits == 1).astype(np.uint8))
    mb = pack_bits_rows((traits != 2).astype(np.uint8))
    p.gm = eng.pack_dense(genes)
    eng.build_lists(p.gm)
    assert p.gm.lists.panels is not None
    p.trv, p.mkv = eng.vecrows(tb, N), eng.vecrows(mb, N)
    p.dense = {}
    cache[key] = p
    return p


def _dense(eng, p, P, seed):
    if (P, seed) not in p.dense:
        res = eng.associate(p.gm, p.trv, p.mkv, permutations=P, seed=seed, use_lists=False)
        p.dense[(P, seed)] = res["r"].cpu().numpy().view(np.uint32).copy()
    return p.dense[(P, seed)]


def _routed(eng, p, P, seed):
    eng.set_mfma_route("all")
    try:
        assert eng.mfma_split(p.gm, p.T, P) == p.G          # every slot on the matrix cores
        res = eng.associate(p.gm, p.trv, p.mkv, permutations=P, seed=seed, use_lists=True)
        return res["r"].cpu().numpy().view(np.uint32).copy()
    finally:
        eng.set_mfma_route("auto")


def _check(eng, cache, G, N, T, P):
    p = _problem(eng, cache, G, N, T)
    want = _dense(eng, p, P, 100 + P)
    got = _routed(eng, p, P, 100 + P)
    assert got.shape == (T, G)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "G %d N %d T %d P %d: %d pairs differ from the dense kernel, first (trait, gene) %s" % (
        G, N, T, P, len(bad), bad[:4].tolist())


def _ranges(eng, G, T, P):
    """[q0, q1) of every range of the launch, in stages of the linear (trait, stage) sequence, and S."""
    import torch
    out = (ctypes.c_int64 * 4)()
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert eng.lib.scoary_mfma_plan(num_cu, G, T, P, out) == 0
    R, L = int(out[1]), int(out[2])
    S = -(-P // 64)
    return [(r * L, min(T * S, (r + 1) * L)) for r in range(R)], S


def _situations(ranges, S):
    found = set()
    for r, (q0, q1) in enumerate(ranges):
        if q0 % S and q1 % S:
            found.add("inside")
        if q0 % S == S - 1:
            found.add("last_is_first")
        if q1 % S == 0 and r < len(ranges) - 1:
            found.add("last_is_last")
        if (q1 - 1) // S - q0 // S >= 2:
            found.add("two_switches")
    return found


@pytest.mark.parametrize("P", [1, 63, 64, 65, 128, 129, 193])
def test_ticks_one_trait(eng, cache, P):
    ranges, S = _ranges(eng, 300, 1, P)
    assert S == -(-P // 64) and sum(q1 - q0 for q0, q1 in ranges) == S
    if P <= 64:
        assert ranges == [(0, 1)]                           # two half stages: intervals 0, 1 and the tail
    _check(eng, cache, 300, 130, 1, P)


# (T, G, P, the situations the case is there for).  The ranges come from the plan for the device's own CU count; the
# cases were chosen on 256 CUs (MI355X), and on a part with another count a case may fail on its situation assert --
# then the shapes have to be chosen anew for that part, r has not been compared.
SWITCHES = [
    (3, 300, 513, {"inside", "last_is_last"}),              # S = 9, ranges of 6
    (3, 300, 1025, {"inside", "last_is_first"}),            # S = 17, ranges of 8: one begins at stage 16
    (5, 300, 513, {"inside", "last_is_last"}),
    (5, 300, 1025, {"inside", "last_is_first"}),
    (3, 40960, 1, {"last_is_first", "two_switches"}),       # S = 1: every stage its trait's last, one range
    (3, 40960, 65, {"two_switches"}),                       # S = 2, one range of 6: switches behind a ragged stage
    (5, 40960, 513, {"inside", "two_switches"}),            # S = 9, three ranges of 15: the middle one both
]


@pytest.mark.parametrize("T,G,P,want", SWITCHES)
def test_trait_switches_at_the_late_boundary(eng, cache, T, G, P, want):
    ranges, S = _ranges(eng, G, T, P)
    found = _situations(ranges, S)
    import torch
    assert want <= found, ("T %d G %d P %d: the plan for this device's %d CUs (the cases were chosen on 256) gives "
                           "ranges %s of S = %d, which have %s, not %s: r was not compared" % (
                               T, G, P, torch.cuda.get_device_properties(0).multi_processor_count, ranges, S,
                               sorted(found), sorted(want)))
    _check(eng, cache, G, 130, T, P)


def test_every_switch_situation_occurs_for_both_trait_counts(eng):
    for T in (3, 5):
        found = set()
        for T2, G, P, _want in SWITCHES:
            if T2 == T:
                found |= _situations(*_ranges(eng, G, T, P))
        assert found == {"inside", "last_is_first", "last_is_last", "two_switches"}, (T, sorted(found))


@pytest.mark.parametrize("G", [33, 129, 160, 256, 257])
def test_slots(eng, cache, G):
    _check(eng, cache, G, 200, 3, 193)


@pytest.mark.parametrize("N", [64, 129, 2000, 2048])
def test_isolates(eng, cache, N):
    _check(eng, cache, 160, N, 3, 129)


def test_same_launch_five_times(eng, cache):
    """Nothing in the barrier / vmcnt structure may depend on timing: five runs, one r."""
    p = _problem(eng, cache, 300, 130, 5, seed=31)
    want = _dense(eng, p, 1025, 9)
    for i in range(5):
        assert np.array_equal(_routed(eng, p, 1025, 9), want), "run %d" % i
