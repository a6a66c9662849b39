"""Labels shuffled within strata (spec S9) on the GPU: k_labels_strata against k_labels for one stratum, against the
plain-Python restatement (strata_spec.py) for several, the tile ranges, the invariants and the per-stratum margins."""
import ctypes

import numpy as np
import pytest

from strata_spec import s9_labels

pytestmark = pytest.mark.gpu
SEED = 0xDEADBEEF12345678


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.close()


def _device_traits(eng, traits):
    """(label rows, validity rows, margins) of a [T, N] trait array with 2 = missing."""
    from scoary_amd.engine import pack_bits_rows
    N = traits.shape[1]
    trv = eng.vecrows(pack_bits_rows((traits == 1).astype(np.uint8)), N)
    mkv = eng.vecrows(pack_bits_rows((traits != 2).astype(np.uint8)), N)
    _, margins = eng.counts(eng.pack_dense(np.ones((1, N), dtype=np.uint8)), trv, mkv)
    return trv, mkv, margins


def _row_bits(rows, N):
    """[T, P, Wp] device rows -> [T, P, N] 0/1; the padding words must be zero."""
    r = rows.cpu().numpy().view(np.uint32)
    assert not r[:, :, 2 * ((N + 63) // 64):].any()
    bits = np.unpackbits(r.view(np.uint8).reshape(r.shape[0], r.shape[1], -1), axis=2, bitorder="little")
    assert not bits[:, :, N:].any()
    return bits[:, :, :N]


def _tile_bits(eng, tiles, T, N, P):
    """Label tiles -> [T, P, N] 0/1, checking the zero row and the zero padding columns on the way."""
    lanes = eng.list_params(N)[0]
    tperm = lanes * 32
    ntiles = -(-P // tperm)
    tw = int(eng.lib.scoary_list_tile_words(N))
    t = tiles.cpu().numpy().view(np.uint32)[:T * ntiles * tw].reshape(T, ntiles, tw)
    t = t[:, :, :(N + 1) * lanes].reshape(T, ntiles, N + 1, lanes)
    out = np.zeros((T, P, N), dtype=np.uint8)
    for ti in range(T):
        for tile in range(ntiles):
            b = np.unpackbits(np.ascontiguousarray(t[ti, tile]).view(np.uint8), axis=1, bitorder="little")
            lo, hi = tile * tperm, min(P, tile * tperm + tperm)
            assert not b[N].any(), "the zero row"
            assert not b[:N, hi - lo:].any(), "padding columns"
            out[ti, lo:hi] = b[:N, :hi - lo].T
    return out


def _random_traits(rng, T, N):
    traits = (rng.random((T, N)) < 0.4).astype(np.uint8)
    traits[0, rng.random(N) < 0.1] = 2
    return traits


@pytest.mark.parametrize("N", [1, 64, 65, 2049, 2600, 5200, 10_300, 20_479])
def test_one_stratum_is_the_unstratified_generator_bit_for_bit(eng, N):
    """strata = zeros: rows and tiles of k_labels_strata equal k_labels' (every list_tw width, more than one row
    per thread, and at the largest N more than 64 KB of LDS per block; row base 5, tile base 32)."""
    T, P = 2, 70
    traits = _random_traits(np.random.default_rng(N), T, N)
    trv, mkv, margins = _device_traits(eng, traits)
    sp = eng.strata_plan(np.zeros(N, dtype=np.int64), trv, mkv, N)
    assert sp.S == 1
    want = eng.perm_generate(mkv, margins, N, P, 5, SEED).cpu().numpy()
    got = eng.perm_generate(mkv, margins, N, P, 5, SEED, strata=sp).cpu().numpy()
    assert np.array_equal(got, want)
    import torch
    words = int(eng.lib.scoary_list_tiles_words(N, P, T))       # (zeroed: a tile ends in up to 3 dwords nobody writes)
    want = eng.perm_generate_tiles(mkv, margins, N, P, 32, SEED,
                                   out=torch.zeros(words, dtype=torch.int32, device=eng.device)).cpu().numpy()
    got = eng.perm_generate_tiles(mkv, margins, N, P, 32, SEED, strata=sp,
                                  out=torch.zeros(words, dtype=torch.int32, device=eng.device)).cpu().numpy()
    assert want.any() or N == 1
    assert np.array_equal(got, want)


def _multipass_case():
    """(N, P, strata, traits, perms) with more strata than a block has lanes per permutation: N = 5000, S = 70 of
    which 60 have members -- six of 1 to 3, two above 300, the rest 40 to 120, all interleaved; trait 0 with missing
    values.  A few blocks of bit rows at this N run 1024 threads = 32 lanes per permutation, so the strata are walked
    in three passes; ``perms`` are the permutations compared with s9_labels."""
    rng = np.random.default_rng(70)
    N, P, S = 5000, 40, 70
    sizes = np.zeros(S, dtype=np.int64)
    live = np.sort(rng.choice(S, 60, replace=False))
    sizes[live] = rng.integers(40, 121, 60)
    sizes[live[[1, 17, 30, 41, 50, 58]]] = [1, 2, 3, 1, 2, 3]
    sizes[live[[5, 47]]] = [350, 420]
    mid, i = [s for s in live if 40 <= sizes[s] <= 120], 0
    while sizes.sum() != N:                                 # the sizes of 40 to 120 take up the remainder in turn
        step = 1 if sizes.sum() < N else -1
        if 40 <= sizes[mid[i % len(mid)]] + step <= 120:
            sizes[mid[i % len(mid)]] += step
        i += 1
    strata = np.repeat(np.arange(S), sizes)[rng.permutation(N)]
    traits = (rng.random((2, N)) < 0.4).astype(np.uint8)
    traits[0, rng.random(N) < 0.1] = 2
    return N, P, strata, traits, (0, 1, 31, 32, 33, P - 1)


def _spec_case(name):
    rng = np.random.default_rng(31)
    if name == "n130":
        # S = 3 with sizes 1, 64 and 65, members interleaved
        N, P, perms = 130, 70, None                          # perms None: every permutation against the restatement
        strata = np.array([1 + (i % 2) for i in range(130)])
        strata[6] = 0
        assert np.bincount(strata).tolist() == [1, 64, 65]
        traits = np.zeros((4, N), dtype=np.uint8)
        traits[0] = rng.random(N) < 0.4                      # ordinary, with missing values
        traits[0, rng.random(N) < 0.12] = 2
        traits[1] = rng.random(N) < 0.3                      # stratum 1 all positive
        traits[1, strata == 1] = 1
        traits[2] = rng.random(N) < 0.5                      # stratum 2 without a valid member
        traits[2, strata == 2] = 2
        traits[3] = rng.random(N) < 0.2                      # npos > nval / 2 in stratum 2 only: the flip per stratum
        traits[3, strata == 2] = rng.random(65) < 0.8
        traits[3, 6] = 0
        assert 2 * int(traits[3, strata == 1].sum()) < 64 and 2 * int(traits[3, strata == 2].sum()) > 65
        return N, P, strata, traits, perms
    if name == "n2100":
        N, P = 2100, 40
        strata = rng.integers(0, 7, N)
        traits = _random_traits(rng, 2, N)
        return N, P, strata, traits, None
    if name == "n5000_three_passes":
        # S = 70 > the 32 lanes a permutation has: the later passes over the strata, with fix-ups of every size
        # (test_strata_spec.py shows from the restatement that the checked permutations have them)
        return _multipass_case()
    N, P = 600, 33                                           # as many strata as the kernel takes: most are empty
    strata = rng.integers(0, 1024, N)
    traits = _random_traits(rng, 2, N)
    return N, P, strata, traits, None


@pytest.mark.parametrize("name", ["n130", "n2100", "n600_max_strata", "n5000_three_passes"])
def test_rows_and_tiles_equal_the_python_restatement(eng, name):
    N, P, strata, traits, perms = _spec_case(name)
    T = traits.shape[0]
    S = {"n600_max_strata": int(eng.lib.scoary_perm_max_strata()), "n5000_three_passes": 70}.get(
        name, int(strata.max()) + 1)
    trait_base = 3
    if name == "n5000_three_passes":
        # the bit rows come from ceil(40 / 32) x 2 traits = 4 blocks: labels_threads(4, 5000, CUs) doubles the block
        # from 256 threads while 4 blocks of it are fewer than 8 wavefronts per CU and a thread keeps >= 4 isolates,
        # so it ends at 1024 threads = 32 lanes per permutation and 70 strata take three passes.  (This holds for the
        # rows, which are what s9_labels is compared with; the tiles may run another block size and must equal them.)
        import torch
        assert 4 * (512 // 64) < 8 * torch.cuda.get_device_properties(0).multi_processor_count and N // 512 >= 4
    trv, mkv, margins = _device_traits(eng, traits)
    sp = eng.strata_plan(strata, trv, mkv, N, S=S)
    rows = _row_bits(eng.perm_generate(mkv, margins, N, P, 0, SEED, trait_base=trait_base, strata=sp), N)
    tiles = _tile_bits(eng, eng.perm_generate_tiles(mkv, margins, N, P, 0, SEED, trait_base=trait_base, strata=sp),
                       T, N, P)
    assert np.array_equal(tiles, rows)
    valid = (traits != 2).astype(int)
    lab = (traits == 1).astype(int)
    for t in range(T):
        for pi in (range(P) if perms is None else perms):
            want = s9_labels(SEED, trait_base + t, pi, valid[t].tolist(), lab[t].tolist(), strata.tolist(), S)
            assert rows[t, pi].tolist() == want, (name, t, pi)
    # rows at a base that is no multiple of 32 are the same permutations
    shifted = _row_bits(eng.perm_generate(mkv, margins, N, P - 7, 7, SEED, trait_base=trait_base, strata=sp), N)
    assert np.array_equal(shifted, rows[:, 7:])


def test_two_columns_per_block_tiles(eng):
    """N = 130, T = 8, P = 4096: 64 tiles of 16 dword columns, enough for two blocks per CU at two columns per
    block, so the tiles come from k_labels_strata<2, 0> (the other cases here launch too few blocks for it).
    They equal the transposed rows, which come from <1, 1>; with one stratum they are k_labels' tiles."""
    import torch
    N, _, strata, four, _ = _spec_case("n130")
    T, P = 8, 4096
    traits = np.concatenate([four, _random_traits(np.random.default_rng(77), T - four.shape[0], N)])
    n_tiles, _tw = eng.tiles_per_batch(N, P, T)
    TW = eng.list_params(N)[0]
    assert (TW, n_tiles) == (16, 64)
    # the launch rule for two columns per block: without this the test would pass through <1, 0> unnoticed
    assert n_tiles * (TW // 2) >= 2 * torch.cuda.get_device_properties(0).multi_processor_count
    trv, mkv, margins = _device_traits(eng, traits)
    sp = eng.strata_plan(strata, trv, mkv, N)
    assert sp.sizes.tolist() == [1, 64, 65]
    rows = _row_bits(eng.perm_generate(mkv, margins, N, P, 0, SEED, strata=sp), N)
    tiles = _tile_bits(eng, eng.perm_generate_tiles(mkv, margins, N, P, 0, SEED, strata=sp), T, N, P)
    assert np.array_equal(tiles, rows)
    assert (rows != (traits == 1)[:, None, :]).any()
    one = eng.strata_plan(np.zeros(N, dtype=np.int64), trv, mkv, N)
    words = int(eng.lib.scoary_list_tiles_words(N, P, T))       # (zeroed: a tile ends in up to 3 dwords nobody writes)
    want = eng.perm_generate_tiles(mkv, margins, N, P, 0, SEED,
                                   out=torch.zeros(words, dtype=torch.int32, device=eng.device)).cpu().numpy()
    got = eng.perm_generate_tiles(mkv, margins, N, P, 0, SEED, strata=one,
                                  out=torch.zeros(words, dtype=torch.int32, device=eng.device)).cpu().numpy()
    assert want.any()
    assert np.array_equal(got, want)


def test_tile_range_halves_concatenate_to_the_whole(eng):
    import torch
    N, T, P = 700, 3, 1100
    rng = np.random.default_rng(8)
    traits = _random_traits(rng, T, N)
    trv, mkv, margins = _device_traits(eng, traits)
    sp = eng.strata_plan(rng.integers(0, 5, N), trv, mkv, N)
    whole = eng.perm_generate_tiles(mkv, margins, N, P, 64, SEED, strata=sp)
    nflat, _tw = eng.tiles_per_batch(N, P, T)
    assert nflat == 9
    whole = whole.clone()
    parts = whole.clone()
    parts[:nflat * _tw] = -1
    eng.perm_generate_tiles(mkv, margins, N, P, 64, SEED, out=parts, tile_range=(0, 4), strata=sp)
    eng.perm_generate_tiles(mkv, margins, N, P, 64, SEED, out=parts, tile_range=(4, 5), strata=sp)
    assert torch.equal(parts, whole)


def test_invariants_and_margins(eng):
    """N = 5000, S = 16, P = 256: per-stratum positive counts, zero row, zero padding, tiles = transposed rows;
    k_strata_margins = numpy."""
    N, T, P, S = 5000, 3, 256, 16
    rng = np.random.default_rng(12)
    traits = _random_traits(rng, T, N)
    traits[2, rng.random(N) < 0.3] = 2
    strata = rng.integers(0, S, N)
    trv, mkv, margins = _device_traits(eng, traits)
    sp = eng.strata_plan(strata, trv, mkv, N)
    want = np.zeros((T, S, 2), dtype=np.int32)
    for s in range(S):
        want[:, s, 0] = (traits[:, strata == s] == 1).sum(1)
        want[:, s, 1] = (traits[:, strata == s] != 2).sum(1)
    assert np.array_equal(sp.smargins.cpu().numpy(), want)
    assert np.array_equal(sp.sizes, np.bincount(strata, minlength=S))
    rows = _row_bits(eng.perm_generate(mkv, margins, N, P, 0, SEED, strata=sp), N)
    tiles = _tile_bits(eng, eng.perm_generate_tiles(mkv, margins, N, P, 0, SEED, strata=sp), T, N, P)
    assert np.array_equal(tiles, rows)
    assert not (rows & (traits == 2)[:, None, :]).any()
    for s in range(S):
        got = rows[:, :, strata == s].sum(2)
        assert np.array_equal(got, np.broadcast_to(want[:, s, 0][:, None], (T, P))), s
    # not the identity shuffle, and not the unstratified labels
    assert (rows != (traits == 1)[:, None, :]).any()
    assert not np.array_equal(rows, _row_bits(eng.perm_generate(mkv, margins, N, P, 0, SEED), N))


def test_largest_shape_the_generator_takes(eng):
    """N = scoary_perm_strata_max_isolates() with scoary_perm_max_strata() strata: the most LDS a block asks for."""
    N, S = int(eng.lib.scoary_perm_strata_max_isolates()), int(eng.lib.scoary_perm_max_strata())
    T, P = 1, 33
    rng = np.random.default_rng(5)
    traits = _random_traits(rng, T, N)
    strata = rng.integers(0, S, N)
    trv, mkv, margins = _device_traits(eng, traits)
    sp = eng.strata_plan(strata, trv, mkv, N, S=S)
    rows = _row_bits(eng.perm_generate(mkv, margins, N, P, 0, SEED, strata=sp), N)
    tiles = _tile_bits(eng, eng.perm_generate_tiles(mkv, margins, N, P, 0, SEED, strata=sp), T, N, P)
    assert np.array_equal(tiles, rows)
    assert not (rows & (traits == 2)[:, None, :]).any()
    want = np.bincount(strata, weights=(traits[0] == 1), minlength=S).astype(np.int64)
    for pi in range(P):
        assert np.array_equal(np.bincount(strata, weights=rows[0, pi], minlength=S).astype(np.int64), want), pi


def test_bad_arguments_return_the_documented_codes(eng):
    import torch
    lib, h = eng.lib, eng.h
    null = ctypes.c_void_p()
    buf = torch.zeros(4096, dtype=torch.int32, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    smax, nmax = int(lib.scoary_perm_max_strata()), int(lib.scoary_perm_strata_max_isolates())
    assert smax >= 256 and nmax == 20479
    gen, til, mar = lib.scoary_perm_generate_strata, lib.scoary_perm_generate_tiles_strata_range, \
        lib.scoary_strata_margins
    assert gen(h, p, p, p, p, null, 1, 10, 1, 4, 0, 0, 1, p, null) == -1              # a null pointer
    assert b"scoary_perm_generate_strata" in lib.scoary_last_error(h)
    assert gen(h, p, p, p, p, p, 1, 10, 0, 4, 0, 0, 1, p, null) == -1                 # no stratum
    assert gen(h, p, p, p, p, p, 70000, 10, 1, 4, 0, 0, 1, p, null) == -3             # T > 65535
    assert gen(h, p, p, p, p, p, 1, 10, 1, 2**33, 0, 0, 1, p, null) == -3             # index >= 2^32
    assert gen(h, p, p, p, p, p, 1, 10, smax + 1, 4, 0, 0, 1, p, null) == -3
    assert b"scoary_perm_max_strata" in lib.scoary_last_error(h)
    assert gen(h, p, p, p, p, p, 1, nmax + 1, 1, 4, 0, 0, 1, p, null) == -3
    assert b"scoary_perm_strata_max_isolates" in lib.scoary_last_error(h)
    assert til(h, p, p, p, p, p, 1, 100, 2, 64, 40, 0, 1, 0, 1, p, null) == -1        # tiles start at a multiple of 32
    assert til(h, p, null, p, p, p, 1, 100, 2, 64, 32, 0, 1, 0, 1, p, null) == -1
    assert til(h, p, p, p, p, p, 2, 100, 2, 600, 0, 0, 1, 3, 2, p, null) == -1        # 2 x 2 tiles: range past the end
    assert til(h, p, p, p, p, p, 1, nmax + 1, 2, 64, 0, 0, 1, 0, 1, p, null) == -3
    assert til(h, p, p, p, p, p, 1, 100, smax + 1, 64, 0, 0, 1, 0, 1, p, null) == -3
    assert til(h, p, p, p, p, p, 1, 100, 2, 64, 2**32, 0, 1, 0, 1, p, null) == -3
    assert mar(h, p, p, null, 1, 10, 1, p, null) == -1
    assert mar(h, p, p, p, 1, 10, smax + 1, p, null) == -3
    assert mar(h, p, p, p, 1, nmax + 1, 1, p, null) == -3
    assert gen(null, p, p, p, p, p, 1, 10, 1, 4, 0, 0, 1, p, null) == -1
    # the offsets are a device array: that they partition [0, N) is the engine's check, on its host copy
    trv, mkv, _ = _device_traits(eng, np.zeros((1, 10), dtype=np.uint8))
    with pytest.raises(ValueError):
        eng.strata_plan(np.zeros(9, dtype=np.int64), trv, mkv, 10)
    with pytest.raises(ValueError):
        eng.strata_plan(np.full(10, -1), trv, mkv, 10)
    with pytest.raises(ValueError):
        eng.strata_plan(np.arange(10), trv, mkv, 10, S=5)
    with pytest.raises(ValueError):
        eng.strata_plan(np.arange(10) * (smax // 9 + 1), trv, mkv, 10)
    sp = eng.strata_plan(np.arange(10) % 3, trv, mkv, 10)
    with pytest.raises(ValueError):
        eng.perm_generate(mkv, None, 11, 4, 0, 1, strata=sp)
    from scoary_amd.engine import StrataPlan
    bad = sp.offsets.clone()
    bad[-1] = 9
    with pytest.raises(ValueError):                     # a plan put together by hand: offsets that do not end at N
        StrataPlan(sp.strata, sp.members, bad, sp.smargins, sp.S, sp.N, sp.sizes)
    twice = sp.members.clone()
    twice[0] = twice[1]
    with pytest.raises(ValueError):
        StrataPlan(sp.strata, twice, sp.offsets, sp.smargins, sp.S, sp.N, sp.sizes)
