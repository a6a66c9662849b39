"""The staggered two-wavefronts-per-SIMD structure of k_permute_mfma at the sizes where it can go wrong.

A block is eight wavefronts of 32 list slots; wavefronts 4..7 run half a stage (16 of its 32 K-steps)
behind 0..3 through a four-slot LDS ring.  Every slot is routed to the matrix
cores and r is compared bit for bit with the dense AND+popcount kernel on every (gene, trait) pair and
with the CPU oracle on 32 genes:

  G = 33   one block whose wavefronts 2..7 own no slot (and wavefront 1 a single one)
  G = 300  two blocks, the second with a partly filled 32-slot wavefront
  G = 513  two full blocks plus one slot
  N        one K-step exactly, one isolate into the second, mid-range, all 32 K-steps
  P = 1    one ragged stage: the late wavefronts' second half has no early work beside it
  P = 64 / 65 / 128 / 129 / 193   one, two and three stages, full or with one permutation in the last,
           the last (ragged) stage being the block's second or first of a pair
  P = 1100 18 stages in three ranges per trait, the last one ragged
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PERMS = (1, 64, 65, 128, 129, 193, 1100)
T = 3


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


def _stagger_problem(G, N, seed):
    """Genes over the whole frequency range, an absent and a core gene, three traits of which two
    have missing values, in different places."""
    rng = np.random.default_rng(seed)
    genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    genes[3] = 0
    genes[4] = 1
    traits = (rng.random((T, N)) < 0.4).astype(np.uint8)
    traits[1, ::29] = 2
    traits[2, 5::17] = 2
    return genes, traits


def _stagger_setup(eng, G, N, seed=23):
    from scoary_amd.engine import pack_bits_rows
    genes, traits = _stagger_problem(G, N, seed)
    tb = pack_bits_rows((traits == 1).astype(np.uint8))
    mb = pack_bits_rows((traits != 2).astype(np.uint8))
    gm = eng.pack_dense(genes)
    eng.build_lists(gm)
    assert gm.lists.panels is not None
    return genes, tb, mb, gm, eng.vecrows(tb, N), eng.vecrows(mb, N)


def _routed_r(eng, gm, trv, mkv, P, seed):
    eng.set_mfma_route("all")
    try:
        assert eng.mfma_split(gm, T, P) == gm.G          # every slot on the matrix cores
        res = eng.associate(gm, trv, mkv, permutations=P, seed=seed, use_lists=True)
        return res["r"].cpu().numpy().view(np.uint32).copy()
    finally:
        eng.set_mfma_route("auto")


@pytest.mark.parametrize("N", [64, 65, 1000, 2048])
@pytest.mark.parametrize("G", [33, 300, 513])
def test_all_routed_equals_dense_and_oracle(eng, G, N):
    from oracle import oracle as orc
    genes, tb, mb, gm, trv, mkv = _stagger_setup(eng, G, N)
    sub = np.unique(np.concatenate([np.arange(0, G, max(1, G // 27))[:27], [3, 4, 31, 32, G - 1]]))[:32]
    gb = orc.pack_rows(genes[sub])
    for P in PERMS:
        seed = 100 + P
        dense = eng.associate(gm, trv, mkv, permutations=P, seed=seed, use_lists=False)
        want = dense["r"].cpu().numpy().view(np.uint32).copy()
        got = _routed_r(eng, gm, trv, mkv, P, seed)
        assert got.shape == (T, G)
        assert np.array_equal(got, want), "P = %d: matrix-core r differs from the dense kernel" % P
        assert np.array_equal(want[:, sub], orc.permute_r(gb, tb, mb, N, P, seed).T), "P = %d: oracle" % P


def test_same_launch_five_times(eng):
    """Nothing in the ring's barrier / vmcnt structure may depend on timing: five runs, one r."""
    genes, tb, mb, gm, trv, mkv = _stagger_setup(eng, 300, 1000)
    dense = eng.associate(gm, trv, mkv, permutations=193, seed=8, use_lists=False)
    want = dense["r"].cpu().numpy().view(np.uint32).copy()
    for i in range(5):
        assert np.array_equal(_routed_r(eng, gm, trv, mkv, 193, 8), want), "run %d" % i
