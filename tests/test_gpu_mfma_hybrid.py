"""The matrix-core kernel of the permutation step (k_permute_mfma) and its routing.

The list slots with the longest lists can take v_mfma_scale_f32_32x32x64_f8f6f4 instead of
the list walk (N <= 2048).  r must be bit-identical whatever is routed: every case below
compares the routed result with the dense AND+popcount kernel (scoary_permute, an
independent implementation) on EVERY (gene, trait) pair and with the CPU oracle on a
gene subsample.
"""
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
def orc():
    from oracle import oracle
    return oracle


def _bits(traits):
    from scoary_amd.engine import pack_bits_rows
    return (pack_bits_rows((traits == 1).astype(np.uint8)),
            pack_bits_rows((traits != 2).astype(np.uint8)))


def _problem(G, N, T=3, seed=11, freq=None):
    """Genes over the whole frequency range (above 0.5: flipped lists), an absent and a core gene
    (skip rule: r == P), traits with two different sets of missing values (mask classes)."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.02, 0.98, (G, 1)) if freq is None else freq
    genes = (rng.random((G, N)) < f).astype(np.uint8)
    if G > 4:
        genes[3] = 0
        genes[4] = 1
    traits = (rng.random((T, N)) < 0.4).astype(np.uint8)
    if T > 1:
        traits[1, ::29] = 2
    if T > 2:
        traits[2, 5::17] = 2
    return genes, traits


def _run(eng, gm, trv, mkv, P, seed, mode, **kw):
    eng.set_mfma_route(mode)
    try:
        res = eng.associate(gm, trv, mkv, permutations=P, seed=seed, use_lists=True, **kw)
        return res["r"].cpu().numpy().view(np.uint32).copy()
    finally:
        eng.set_mfma_route("auto")


def _k_split(eng, gm, T, P, mode):
    eng.set_mfma_route(mode)
    try:
        return eng.mfma_split(gm, T, P)
    finally:
        eng.set_mfma_route("auto")


def _check(eng, orc, genes, traits, P, seed, sub, modes=("all",), **kw):
    G, N = genes.shape
    T = traits.shape[0]
    tb, mb = _bits(traits)
    gm = eng.pack_dense(genes)
    eng.build_lists(gm)
    trv, mkv = eng.vecrows(tb, N), eng.vecrows(mb, N)
    dense = eng.associate(gm, trv, mkv, permutations=P, seed=seed, use_lists=False)
    want = dense["r"].cpu().numpy().view(np.uint32).copy()
    counts = dense["counts"].cpu().numpy()
    got = {}
    for mode in modes:
        got[mode] = _run(eng, gm, trv, mkv, P, seed, mode, **kw)
        assert np.array_equal(got[mode], want), "routing %r differs from the dense kernel" % mode
    gb = orc.pack_rows(genes[sub])
    assert np.array_equal(want[:, sub], orc.permute_r(gb, tb, mb, N, P, seed).T)
    skipped = (counts[:, :, 0] + counts[:, :, 2] == 0) | (counts[:, :, 1] + counts[:, :, 3] == 0)
    assert np.all(want[skipped] == P)
    return gm, trv, mkv, want


def test_cfg3_routing_auto_all_none(eng):
    """cfg3 (the headline shape): routing auto, all and none give the same r, equal to the dense
    kernel on all 500 000 pairs; auto does route whole 256-slot blocks of the long-list end."""
    from scoary_amd import synth
    genes, traits, P, seed = synth.make_config("cfg3")
    G, N = genes.shape
    T = traits.shape[0]
    tb, mb = _bits(traits)
    gm = eng.pack_dense(genes)
    eng.build_lists(gm)
    assert gm.lists.panels is not None
    k_auto = _k_split(eng, gm, T, P, "auto")
    assert 0 < k_auto < G and k_auto % 256 == 0
    assert _k_split(eng, gm, T, P, "all") == G and _k_split(eng, gm, T, P, "none") == 0
    trv, mkv = eng.vecrows(tb, N), eng.vecrows(mb, N)
    dense = eng.associate(gm, trv, mkv, permutations=P, seed=seed, use_lists=False)
    want = dense["r"].cpu().numpy().view(np.uint32).copy()
    for mode in ("auto", "all", "none"):
        assert np.array_equal(_run(eng, gm, trv, mkv, P, seed, mode), want), mode


@pytest.mark.parametrize("N", [65, 1999, 2000, 2048])
@pytest.mark.parametrize("P", [1, 63, 1000])
def test_all_routed_shapes(eng, orc, N, P):
    """Every slot on the matrix cores: G = 1000 is neither a multiple of 64 nor of 256 (a partly filled
    wave panel and block), N at and around the K-step and row limits, P with a ragged last stage."""
    genes, traits = _problem(1000, N)
    _check(eng, orc, genes, traits, P, 77, np.arange(0, 1000, 16), modes=("all", "none"))


def test_full_permutation_count(eng, orc):
    """P = 10 000 (157 stages, the last one ragged) with 700 genes, all routed."""
    genes, traits = _problem(700, 2000, T=2)
    _check(eng, orc, genes, traits, 10_000, 5, np.arange(0, 700, 50))


def test_balanced_matrix_auto_routes_everything(eng, orc):
    """Every gene at frequency 0.5 (the longest lists there are): auto routes every whole block."""
    G, N, T, P = 8192, 2000, 4, 2048
    genes, traits = _problem(G, N, T=T, freq=0.5)
    gm, trv, mkv, want = _check(eng, orc, genes, traits, P, 3, np.arange(0, G, 512), modes=("auto", "all"))
    assert _k_split(eng, gm, T, P, "auto") == G


def test_fewer_genes_than_one_block(eng, orc):
    genes, traits = _problem(37, 333)
    _check(eng, orc, genes, traits, 200, 9, np.arange(37))


def test_not_routed_above_2048_isolates(eng, orc):
    """N = 2049 needs a 33rd K-step: no panels, k_split = 0 in every mode, r as ever."""
    genes, traits = _problem(600, 2049)
    gm, trv, mkv, want = _check(eng, orc, genes, traits, 300, 21, np.arange(0, 600, 20), modes=("all", "auto"))
    assert gm.lists.panels is None
    assert _k_split(eng, gm, 3, 300, "all") == 0


def test_second_label_batch_accumulates(eng, orc):
    """P above one label batch: the second batch adds to r (accumulate) through both kernels."""
    genes, traits = _problem(1500, 2000)
    G, N = genes.shape
    P, seed = 1000, 13
    tb, mb = _bits(traits)
    gm = eng.pack_dense(genes)
    eng.build_lists(gm)
    trv, mkv = eng.vecrows(tb, N), eng.vecrows(mb, N)
    dense = eng.associate(gm, trv, mkv, permutations=P, seed=seed, use_lists=False)
    want = dense["r"].cpu().numpy().view(np.uint32).copy()
    ws = eng.workspace(gm, traits.shape[0], P, use_lists=True)
    ws.batch = 512                        # two batches: 512 + 488 permutations
    for mode in ("all", "none"):
        assert np.array_equal(_run(eng, gm, trv, mkv, P, seed, mode, workspace=ws, graph=False), want), mode
    sub = np.arange(0, G, 100)
    assert np.array_equal(want[:, sub], orc.permute_r(orc.pack_rows(genes[sub]), tb, mb, N, P, seed).T)


def test_captured_step_and_auto_graph_replay(eng):
    """engine.capture and the automatic graph replay of launch-bound shapes give the eager r with
    routed slots: the matrix-core kernels run on the main stream, in sequence with the list kernel."""
    import torch
    genes, traits = _problem(900, 500, T=2)
    G, N = genes.shape
    T, P, seed = 2, 500, 4
    tb, mb = _bits(traits)
    gm = eng.pack_dense(genes)
    eng.build_lists(gm)
    trv, mkv = eng.vecrows(tb, N), eng.vecrows(mb, N)
    eng.set_mfma_route("all")
    try:
        want = eng.associate(gm, trv, mkv, permutations=P, seed=seed, use_lists=False)["r"].cpu().numpy().copy()
        ws = eng.workspace(gm, T, P, use_lists=True)
        plan = eng.trait_plan(trv, mkv, N)
        graph, res = eng.capture(gm, trv, mkv, P, seed, ws, use_lists=True, plan=plan)
        res["r"].zero_()
        graph.launch()
        torch.cuda.synchronize()
        assert np.array_equal(res["r"].cpu().numpy(), want)
        graph.close()
        ws2 = eng.workspace(gm, T, P, use_lists=True)
        assert eng.auto_graph_eligible(gm, T, P)
        for _ in range(4):                # eager, record, replay, replay
            res = eng.associate(gm, trv, mkv, permutations=P, seed=seed, use_lists=True, workspace=ws2, plan=plan)
            torch.cuda.synchronize()
            assert np.array_equal(res["r"].cpu().numpy(), want)
    finally:
        eng.set_mfma_route("auto")
