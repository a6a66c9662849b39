"""The label generator's output mode "tiles + fragments": the B fragments of k_permute_mfma written by k_labels /
k_labels_strata next to their tile rows (scoary_perm_generate_tiles_bfrag_range and its strata sibling) instead of
by a conversion pass over the tiles (k_mfma_bfrag).

Everything is compared byte for byte, nothing has a tolerance.  The reference of the fragments is what k_mfma_bfrag
-- scoary_permute_hybrid with every slot routed and bfrag_ready = 0 -- makes of the same call's tiles; a numpy
restatement of the layout (bfrag[t][s][k][j][lane] x 16 bytes, include/scoary_hip.h and mfma_bfrag_emit) checks
that reference in turn.  The step-level cases compare associate() with the fused path against the same call with
engine.fuse_bfrag = False.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20240611
CANARY = 4096          # int32 words behind the fragment buffer that no kernel may touch
N_CASES = (1, 63, 130, 2000, 2048)          # rows past N in a K-step, a partial K-step, the full width
P_CASES = (1, 64, 100, 513, 1100)           # a ragged stage, dead stages in the last tile, more than one tile


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.set_mfma_route("auto")
    e.fuse_bfrag = True
    e.close()


@pytest.fixture(scope="module")
def cache():
    return {}


def _traits(T, N, seed=3):
    """Trait 0 with more positives than half its valid isolates (row_field's flip branch), trait 1 with missing
    values, the others plain."""
    rng = np.random.default_rng(seed + N)
    traits = (rng.random((T, N)) < 0.4).astype(np.uint8)
    traits[0] = (rng.random(N) < 0.8).astype(np.uint8)
    traits[0, 0] = 1
    if T > 1:
        traits[1, ::7] = 2
    return traits


def _device_traits(eng, traits):
    from scoary_amd.engine import pack_bits_rows
    N = traits.shape[1]
    trv = eng.vecrows(pack_bits_rows((traits == 1).astype(np.uint8)), N)
    mkv = eng.vecrows(pack_bits_rows((traits != 2).astype(np.uint8)), N)
    _, margins = eng.counts(eng.pack_dense(np.ones((1, N), dtype=np.uint8)), trv, mkv)
    return trv, mkv, margins


def _setup(eng, cache, T, N):
    """Per (T, N), once: the traits on the device and a small gene matrix with lists and panels, which is what
    scoary_permute_hybrid needs to run k_mfma_bfrag on a set of tiles."""
    key = (T, N)
    if key not in cache:
        traits = _traits(T, N)
        assert 2 * int((traits[0] == 1).sum()) > int((traits[0] != 2).sum())
        trv, mkv, margins = _device_traits(eng, traits)
        genes = (np.random.default_rng(N).random((40, N)) < 0.5).astype(np.uint8)
        gm = eng.pack_dense(genes)
        eng.build_lists(gm)
        assert gm.lists.panels is not None
        cache[key] = (traits, trv, mkv, margins, gm)
    return cache[key]


def _buffers(eng, N, P, T):
    import torch
    words = int(eng.lib.scoary_list_tiles_words(N, P, T))
    fwords = int(eng.lib.scoary_mfma_bfrag_bytes(N, P, T)) // 4
    assert fwords == T * (-(-P // 64)) * 16384
    tiles = torch.zeros(words, dtype=torch.int32, device=eng.device)       # (a tile ends in dwords nobody writes)
    frag = torch.full((fwords + CANARY,), -1, dtype=torch.int32, device=eng.device)
    return tiles, frag, fwords


def _fragments_by_conversion(eng, gm, tiles, margins, N, P, T):
    """What k_mfma_bfrag makes of ``tiles``: one scoary_permute_hybrid call with every slot routed."""
    import torch
    fwords = int(eng.lib.scoary_mfma_bfrag_bytes(N, P, T)) // 4
    frag = torch.full((fwords + CANARY,), -1, dtype=torch.int32, device=eng.device)
    crit = torch.zeros((T, gm.G, 2), dtype=torch.int32, device=eng.device)
    r = torch.zeros((T, gm.G), dtype=torch.int32, device=eng.device)
    eng.set_mfma_route("all")
    try:
        assert eng.mfma_split(gm, T, P) == gm.G
        eng.permute_lists(gm, tiles, crit, margins, P, r, accumulate=False, bfrag=frag, bfrag_ready=False)
    finally:
        eng.set_mfma_route("auto")
    out = frag.cpu().numpy()
    assert np.all(out[fwords:] == -1)
    return out[:fwords].copy()


def _fragments_by_numpy(eng, tiles, T, N, P):
    """The layout restated: lane l of fragment (t, s, k, j) holds permutation 64 s + 32 j + (l & 31) and the isolates
    64 k + 32 (l >> 5) .. + 31, one E2M1 nibble each (0x2 = 1.0), the even isolate in the low nibble of a byte."""
    tw = int(eng.lib.scoary_list_tile_words(N))
    ntiles, S = -(-P // 512), -(-P // 64)
    t = tiles.cpu().numpy().view(np.uint32)[:T * ntiles * tw].reshape(T, ntiles, tw)[:, :, :N * 16]
    rows = np.ascontiguousarray(t.reshape(T, ntiles, N, 16))
    bits = np.unpackbits(rows.view(np.uint8), axis=3, bitorder="little")          # [T, tile, isolate, 512]
    lab = np.zeros((T, ntiles * 512, 2048), dtype=np.uint8)                       # [T, permutation, isolate]
    lab[:, :, :N] = bits.transpose(0, 1, 3, 2).reshape(T, ntiles * 512, N)
    lab = lab[:, :S * 64].reshape(T, S, 2, 32, 32, 2, 16, 2)                      # t s j l31 k half byte nibble
    lab = lab.transpose(0, 1, 4, 2, 5, 3, 6, 7)                                   # t s k j half l31 byte nibble
    by = (lab[..., 0] * 0x02 + lab[..., 1] * 0x20).astype(np.uint8)
    return np.ascontiguousarray(by).reshape(-1).view(np.int32)


def _nb(eng, nflat):
    """The generator's shape rule (tile_shape): two dword columns per block from two blocks per CU on."""
    import torch
    num_cu = torch.cuda.get_device_properties(eng.device).multi_processor_count
    return 2 if nflat * 8 >= 2 * num_cu else 1


def _compare(eng, cache, T, N, P, base, strata=None, window=None):
    """Fused against unfused + conversion for one launch; returns the fused fragments (int32 words)."""
    traits, trv, mkv, margins, gm = _setup(eng, cache, T, N)
    nflat = T * (-(-P // 512))
    kw = {"strata": strata, "tile_range": window}
    plain, _unused, _ = _buffers(eng, N, P, T)
    eng.perm_generate_tiles(mkv, margins, N, P, base, SEED, out=plain, **kw)
    tiles, frag, fwords = _buffers(eng, N, P, T)
    eng.perm_generate_tiles(mkv, margins, N, P, base, SEED, out=tiles, bfrag=frag, **kw)
    got = frag.cpu().numpy()
    what = "N=%d P=%d base=%d window=%s" % (N, P, base, window)
    assert np.all(got[fwords:] == -1), "canary behind the fragments, " + what
    assert np.array_equal(tiles.cpu().numpy(), plain.cpu().numpy()), "tiles, " + what
    want = _fragments_by_conversion(eng, gm, tiles, margins, N, P, T)
    if window is None:
        assert np.array_equal(want, _fragments_by_numpy(eng, tiles, T, N, P)), "k_mfma_bfrag vs the layout, " + what
        assert want.any() or N == 1
    else:
        # stages of (trait, tile) cells outside the window keep the fill
        S = -(-P // 64)
        ntiles = -(-P // 512)
        keep = np.ones((T, S), dtype=bool)
        for f in range(window[0], window[0] + window[1]):
            keep[f // ntiles, (f % ntiles) * 8:(f % ntiles) * 8 + 8] = False
        assert keep.any() and not keep.all()
        want = want.reshape(T, S, -1).copy()
        want[keep] = -1
        want = want.reshape(-1)
    assert np.array_equal(got[:fwords], want), "fragments, " + what
    return got[:fwords].copy()


@pytest.mark.parametrize("base", [0, 1024])
@pytest.mark.parametrize("N", N_CASES)
def test_fused_fragments_equal_the_conversion(eng, cache, N, base):
    for P in P_CASES:
        assert _nb(eng, 3 * (-(-P // 512))) == 1
        _compare(eng, cache, 3, N, P, base)


@pytest.mark.parametrize("N", [63, 2048])
def test_tile_window_leaves_the_other_stages_alone(eng, cache, N):
    """P = 1100: three tiles per trait, the last with two live stages; the window covers the end of trait 0 and
    the whole of trait 1, so trait 2 and the first two tiles of trait 0 keep the 0xFF fill."""
    _compare(eng, cache, 3, N, 1100, 1024, window=(2, 4))


def test_two_columns_per_block(eng, cache):
    """64 flat tiles x 8 units >= 2 x 256 CUs: the launch takes NB = 2, a block writes a whole stage (every other
    case here has too few blocks and runs NB = 1)."""
    T, N, P = 8, 130, 4096
    assert _nb(eng, T * (P // 512)) == 2
    _compare(eng, cache, T, N, P, 0)


@pytest.mark.parametrize("S", [1, 3])
def test_strata_generator(eng, cache, S):
    T, N, P = 3, 130, 513
    traits, trv, mkv, margins, gm = _setup(eng, cache, T, N)
    sp = eng.strata_plan(np.arange(N, dtype=np.int64) % S, trv, mkv, N)
    assert sp.S == S
    got = _compare(eng, cache, T, N, P, 0, strata=sp)
    if S == 1:
        assert np.array_equal(got, _compare(eng, cache, T, N, P, 0)), "one stratum: the plain generator's fragments"


@pytest.mark.parametrize("N", [2049, 2600])      # a 33rd K-step; eight-dword tiles (list_tw(N) = 8)
def test_refused_shapes_write_nothing(eng, N):
    import torch
    T, P = 2, 100
    assert eng.list_params(N)[0] == (16 if N == 2049 else 8)
    traits = _traits(T, N)
    trv, mkv, margins = _device_traits(eng, traits)
    sp = eng.strata_plan(np.zeros(N, dtype=np.int64), trv, mkv, N)
    tiles = torch.full((int(eng.lib.scoary_list_tiles_words(N, P, T)),), -1, dtype=torch.int32, device=eng.device)
    frag = torch.full((T * 2 * 16384,), -1, dtype=torch.int32, device=eng.device)
    assert int(eng.lib.scoary_mfma_bfrag_bytes(N, P, T)) == 0
    nflat = eng.tiles_per_batch(N, P, T)[0]
    rc = eng.lib.scoary_perm_generate_tiles_bfrag_range(
        eng.h, eng._ptr(mkv), eng._ptr(margins), T, N, P, 0, 0, ctypes.c_uint64(SEED), 0, nflat, eng._ptr(tiles),
        eng._ptr(frag), eng._stream())
    assert rc == -3, rc                                        # SCOARY_ERR_SIZE
    rc = eng.lib.scoary_perm_generate_tiles_strata_bfrag_range(
        eng.h, eng._ptr(mkv), *eng._strata_ptrs(sp), T, N, 1, P, 0, 0, ctypes.c_uint64(SEED), 0, nflat,
        eng._ptr(tiles), eng._ptr(frag), eng._stream())
    assert rc == -3, rc
    torch.cuda.synchronize()
    assert bool((tiles == -1).all()) and bool((frag == -1).all())


# ---------------------------------------------------------------------------------------- the step
def _step_problem(eng, cache, G, N, T):
    key = ("step", G, N, T)
    if key not in cache:
        from scoary_amd.engine import pack_bits_rows
        rng = np.random.default_rng(G + N)
        genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
        genes[3], genes[4] = 0, 1
        traits = _traits(T, N)
        gm = eng.pack_dense(genes)
        eng.build_lists(gm)
        assert gm.lists.panels is not None
        trv = eng.vecrows(pack_bits_rows((traits == 1).astype(np.uint8)), N)
        mkv = eng.vecrows(pack_bits_rows((traits != 2).astype(np.uint8)), N)
        cache[key] = (gm, trv, mkv)
    return cache[key]


def _step(eng, fuse, gm, trv, mkv, P, keys=("r", "p", "crit"), batch=None, **kw):
    """One associate() with the fused path on or off -> the named results as host arrays, and whether the step
    launched k_mfma_bfrag (the library's kernel timers)."""
    import torch
    from scoary_amd import _abi
    eng.fuse_bfrag = fuse
    try:
        ws = eng.workspace(gm, trv.shape[0], P, use_lists=True)
        if batch:
            ws.batch = batch
        eng.set_timing(True)
        res = eng.associate(gm, trv, mkv, permutations=P, seed=SEED, use_lists=True, workspace=ws, **kw)
        torch.cuda.synchronize()
        try:
            eng.kernel_ms("k_mfma_bfrag")
            converted = True
        except _abi.ScoaryHipError:
            converted = False
        return {k: res[k].cpu().numpy().copy() for k in keys}, converted
    finally:
        eng.set_timing(False)
        eng.fuse_bfrag = True


def _same_step(eng, gm, trv, mkv, P, **kw):
    a, conv_a = _step(eng, True, gm, trv, mkv, P, **kw)
    b, conv_b = _step(eng, False, gm, trv, mkv, P, **kw)
    assert not conv_a and conv_b, "the fused step converts nothing, the unfused one does"
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    return a


def test_step_route_all(eng, cache):
    gm, trv, mkv = _step_problem(eng, cache, 600, 2000, 3)
    eng.set_mfma_route("all")
    try:
        res = _same_step(eng, gm, trv, mkv, 1100)
    finally:
        eng.set_mfma_route("auto")
    dense = eng.associate(gm, trv, mkv, permutations=1100, seed=SEED, use_lists=False)
    assert np.array_equal(res["r"], dense["r"].cpu().numpy())


def test_step_forced_split_at_256_slots(eng, cache, monkeypatch):
    gm, trv, mkv = _step_problem(eng, cache, 600, 1000, 3)
    monkeypatch.setattr(eng, "mfma_split", lambda genes, T, P: 256)
    _same_step(eng, gm, trv, mkv, 1100)


def test_step_second_label_batch(eng, cache):
    """P above the label batch: the second batch (488 permutations: fewer stages per trait, the fragments of the
    first batch still behind them in the buffer) accumulates."""
    gm, trv, mkv = _step_problem(eng, cache, 600, 2000, 3)
    eng.set_mfma_route("all")
    try:
        two = _same_step(eng, gm, trv, mkv, 1000, batch=512, graph=False)
        one, _ = _step(eng, True, gm, trv, mkv, 1000)
    finally:
        eng.set_mfma_route("auto")
    assert np.array_equal(two["r"], one["r"])


def test_step_captured_graph_replay(eng, cache):
    import torch
    gm, trv, mkv = _step_problem(eng, cache, 600, 500, 3)
    T, P = 3, 500
    eng.set_mfma_route("all")
    try:
        want, _ = _step(eng, False, gm, trv, mkv, P)
        ws = eng.workspace(gm, T, P, use_lists=True)
        plan = eng.trait_plan(trv, mkv, gm.N)
        graph, res = eng.capture(gm, trv, mkv, P, SEED, ws, use_lists=True, plan=plan)
        res["r"].zero_()
        ws.bfrag.fill_(-1)
        graph.launch()
        torch.cuda.synchronize()
        for k in want:
            assert res[k].cpu().numpy().tobytes() == want[k].tobytes(), k
        graph.close()
        ws2 = eng.workspace(gm, T, P, use_lists=True)
        assert eng.auto_graph_eligible(gm, T, P)
        for _ in range(4):                # eager, record, replay, replay
            res = eng.associate(gm, trv, mkv, permutations=P, seed=SEED, use_lists=True, workspace=ws2, plan=plan)
            torch.cuda.synchronize()
            assert np.array_equal(res["r"].cpu().numpy(), want["r"])
    finally:
        eng.set_mfma_route("auto")


def test_step_cmh_counts_both_regions_on_one_set_of_fragments(eng, cache):
    gm, trv, mkv = _step_problem(eng, cache, 600, 1000, 3)
    sp = eng.strata_plan(np.arange(gm.N, dtype=np.int64) % 4, trv, mkv, gm.N)
    eng.set_mfma_route("all")
    try:
        _same_step(eng, gm, trv, mkv, 1100, keys=("r", "r_cmh", "p", "crit"), strata=sp, cmh=True)
    finally:
        eng.set_mfma_route("auto")
