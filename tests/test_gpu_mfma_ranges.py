"""k_permute_mfma over ranges of the linear (trait, stage) sequence: blocks that serve several traits, and
ranges that start and end inside a trait.

Every slot is routed to the matrix cores; r is compared bit for bit with the dense AND+popcount kernel on every
(gene, trait) pair and with the CPU oracle on 32 genes.  Each case first asserts, through scoary_mfma_plan with
the device's CU count, that the launch has the property the case is for (a plan without it fails the case):

  (a) several whole traits in one block   G = 65 536, N = 130, T = 3, P = 193: S = 4 stages per trait and one
      partial tile, so a cut is admissible on a trait boundary only; one range of 12 stages per gene block, 256
      blocks: each block ends two segments inside its loop and one behind it, the last stage of every trait
      ragged (one permutation)
  (b) ranges that cut a trait             G = 32 768, N = 200, P = 1100 (S = 18, last stage of 12) and P = 1152
      (last stage full), three partial tiles.  T = 3: two ranges of 27 stages, trait 1 cut after its stage 8 --
      range 0 writes tile 0 of trait 1, range 1 tile 1 and the zeros of tile 2.  T = 5: two ranges of 45, trait 2
      cut in the middle, three traits per block
  (c) repeatability                       case (b) five times, one r
  (d) poisoned scratch                    case (b) with the partial counts (and the B fragments) filled with 0xFF
      before the launch: a (trait, tile) cell that no segment writes, or a zero tile left out, shows in r
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


def _plan(eng, G, T, P):
    import torch
    out = (ctypes.c_int64 * 4)()
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert eng.lib.scoary_mfma_plan(num_cu, G, T, P, out) == 0
    return {"gene_blocks": int(out[0]), "R": int(out[1]), "L": int(out[2]), "blocks": int(out[3])}


class Problem:
    pass


def _problem(eng, cache, G, N, T, seed=23):
    """Genes over the whole frequency range, an absent and a core gene; traits 1 and 2 (and 4) have missing
    values, in different places."""
    key = (G, N, T)
    if key in cache:
        return cache[key]
    from scoary_amd.engine import pack_bits_rows
    rng = np.random.default_rng(seed)
    p = Problem()
    p.G, p.N, p.T = G, N, T
    p.genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    p.genes[3] = 0
    p.genes[4] = 1
    traits = (rng.random((T, N)) < 0.4).astype(np.uint8)
    traits[1, ::29] = 2
    traits[2, 5::17] = 2
    if T > 4:
        traits[4, 2::11] = 2
    p.tb = pack_bits_rows((traits == 1).astype(np.uint8))
    p.mb = pack_bits_rows((traits != 2).astype(np.uint8))
    p.gm = eng.pack_dense(p.genes)
    eng.build_lists(p.gm)
    assert p.gm.lists.panels is not None
    p.trv, p.mkv = eng.vecrows(p.tb, N), eng.vecrows(p.mb, N)
    p.sub = np.unique(np.concatenate([np.arange(0, G, max(1, G // 27))[:27], [3, 4, 31, 32, G - 1]]))[:32]
    p.dense = {}
    cache[key] = p
    return p


def _dense(eng, p, P, seed):
    """The dense kernel's r of (P, seed), checked once against the CPU oracle on 32 genes."""
    if (P, seed) not in p.dense:
        from oracle import oracle as orc
        res = eng.associate(p.gm, p.trv, p.mkv, permutations=P, seed=seed, use_lists=False)
        want = res["r"].cpu().numpy().view(np.uint32).copy()
        gb = orc.pack_rows(p.genes[p.sub])
        assert np.array_equal(want[:, p.sub], orc.permute_r(gb, p.tb, p.mb, p.N, P, seed).T), "dense against oracle"
        p.dense[(P, seed)] = want
    return p.dense[(P, seed)]


def _routed(eng, p, P, seed, workspace=None):
    eng.set_mfma_route("all")
    try:
        assert eng.mfma_split(p.gm, p.T, P) == p.G          # every slot on the matrix cores
        res = eng.associate(p.gm, p.trv, p.mkv, permutations=P, seed=seed, use_lists=True, workspace=workspace,
                            graph=False)
        return res["r"].cpu().numpy().view(np.uint32).copy()
    finally:
        eng.set_mfma_route("auto")


def _assert_cut_plan(eng, G, T, P):
    """Case (b): two ranges per gene block, the cut strictly inside a trait."""
    S = -(-P // 64)
    plan = _plan(eng, G, T, P)
    assert plan["R"] == 2 and plan["L"] == -(-T * S // 2), plan
    assert plan["L"] % S != 0 and plan["L"] > S, plan       # starts and ends inside a trait, enters another
    return plan


def test_several_whole_traits_in_one_block(eng, cache):
    G, N, T, P = 65536, 130, 3, 193
    plan = _plan(eng, G, T, P)
    assert plan["R"] == 1 and plan["L"] == T * 4 and plan["blocks"] == G // 256, plan
    p = _problem(eng, cache, G, N, T)
    want = _dense(eng, p, P, 100 + P)
    got = _routed(eng, p, P, 100 + P)
    assert got.shape == (T, G)
    assert np.array_equal(got, want), "matrix-core r differs from the dense kernel"


@pytest.mark.parametrize("P", [1100, 1152])
@pytest.mark.parametrize("T", [3, 5])
def test_ranges_that_cut_a_trait(eng, cache, T, P):
    G, N = 32768, 200
    _assert_cut_plan(eng, G, T, P)
    p = _problem(eng, cache, G, N, T)
    want = _dense(eng, p, P, 100 + P)
    got = _routed(eng, p, P, 100 + P)
    assert got.shape == (T, G)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "T = %d P = %d: %d pairs differ from the dense kernel, first (trait, gene) %s" % (
        T, P, len(bad), bad[:4].tolist())


def test_same_launch_five_times(eng, cache):
    """Nothing in the trait switch may depend on timing: five runs, one r."""
    G, N, T, P = 32768, 200, 3, 1100
    _assert_cut_plan(eng, G, T, P)
    p = _problem(eng, cache, G, N, T)
    want = _dense(eng, p, P, 100 + P)
    for i in range(5):
        assert np.array_equal(_routed(eng, p, P, 100 + P), want), "run %d" % i


@pytest.mark.parametrize("T", [3, 5])
def test_poisoned_scratch(eng, cache, T):
    G, N, P = 32768, 200, 1100
    _assert_cut_plan(eng, G, T, P)
    p = _problem(eng, cache, G, N, T)
    want = _dense(eng, p, P, 100 + P)
    ws = eng.workspace(p.gm, T, P, use_lists=True)
    ws.scratch.fill_(-1)
    ws.bfrag.fill_(-1)
    assert np.array_equal(_routed(eng, p, P, 100 + P, workspace=ws), want)
