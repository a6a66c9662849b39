"""The Hodges-Lehmann shift of the rank-sum test and its confidence limits (spec S19) on the GPU, through the raw
entry point and the engine, against the restatement rank_shift_spec.py: shift, lower, upper and ca bit for bit.

Shapes: n = 2, 3, 4 with every gene there is; N at the edges of a word and of a wavefront's 64 places; missing
values; every N at which a block changes its number of wavefronts (scoary_rank_shift_waves) and one past it; heavy
ties; all-distinct values over three traits; G at the edges of a round of 16 genes and of 256; m = 1, 2, n - 2,
n - 1; genes next to their complements; N = 16 320 with m = 8 160 (K = 66 585 600); the levels 0.5, 0.95 and 0.999;
untestable genes and traits.

ca: the device takes sqrt and floor itself.  No cell of these cases has the spec's unfloored value within 1e-9
(relative, of at least 1) of an integer -- asserted for every cell -- so ca is held exactly, and the limits with it.

test_gpu_rank_shift_limits.py goes on where these stop: several genes per wavefront, values from subnormals to 1e150,
traits of no, one and two values."""
import ctypes
import math

import numpy as np
import pytest

import rank_shift_spec as spec

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_SIZE = -1, -3           # SCOARY_ERR_ARG, SCOARY_ERR_SIZE of include/scoary_hip.h
MAX_N = 16320


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.close()


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _run(eng, vals, genes, level):
    gm = eng.pack_dense(np.ascontiguousarray(genes, dtype=np.uint8))
    plan = eng.ranksum_plan(vals)
    res = eng.ranksum(gm, plan)
    out = eng.ranksum_shift(gm, plan, res, level=level)
    return {k: v.cpu().numpy() for k, v in out.items()}, res["m"].cpu().numpy()


def _check(eng, vals, genes, level=0.95, partition=False, want_infinite=None):
    """Every (trait, gene) against the restatement, bit for bit.  Returns how many cells have limits."""
    vals = np.asarray(vals, dtype=np.float64)
    got, m = _run(eng, vals, genes, level)
    T, G = vals.shape[0], genes.shape[0]
    assert all(got[k].shape == (T, G) for k in ("shift", "lower", "upper", "ca"))
    finite = 0
    for t in range(T):
        for g in range(G):
            shift, lower, upper, ca, raw = spec.shift_spec(vals[t], genes[g], level, partition=partition)
            assert abs(raw - round(raw)) > 1e-9 * max(abs(raw), 1.0) or raw == 0.0, (t, g, raw)
            where = (t, g, int(m[t, g]))
            assert int(got["ca"][t, g]) == ca, where
            for key, want in (("shift", shift), ("lower", lower), ("upper", upper)):
                assert _bits(got[key][t, g]) == _bits(want), (key,) + where + (got[key][t, g], want)
            finite += ca >= 1
    if want_infinite is not None:
        assert (finite < T * G) == want_infinite
    return finite


def _edge_genes(rng, N, extra=6):
    """m = 0, n, 1, 2, N - 2, N - 1 (of all isolates), a random gene and its complement, and ``extra`` more."""
    rows = [np.zeros(N, bool), np.ones(N, bool)]
    for m in (1, 2, N - 2, N - 1):
        r = np.zeros(N, bool)
        r[rng.permutation(N)[:max(m, 0)]] = True
        rows.append(r)
    r = rng.random(N) < 0.3
    rows += [r, ~r]
    rows += [rng.random(N) < f for f in rng.uniform(0.05, 0.95, extra)]
    return np.array(rows)


def test_two_three_and_four_isolates_every_gene(eng):
    for n in (2, 3, 4):
        genes = np.array([[(g >> i) & 1 for i in range(n)] for g in range(1 << n)], dtype=np.uint8)
        vals = np.array([[0.5, -1.25, 3.0, 3.0][:n], [4.0, 1.0, 2.0, 8.0][:n]])
        _check(eng, vals, genes, 0.95, want_infinite=True)          # n = 4, m = 2 at 95 %: no interval
        _check(eng, vals, genes, 0.5)


@pytest.mark.parametrize("N", (31, 32, 33, 63, 64, 65))
def test_word_and_wavefront_edges(eng, N):
    rng = np.random.default_rng(N)
    vals = np.stack([np.round(rng.standard_normal(N), 1), rng.standard_normal(N)])
    assert _check(eng, vals, _edge_genes(rng, N)) > 10


def test_missing_values_and_a_ragged_last_word(eng):
    rng = np.random.default_rng(7)
    N = 77
    vals = np.stack([np.exp2(rng.integers(-3, 4, N).astype(float)), rng.standard_normal(N) * 1e-3,
                     rng.standard_normal(N)])
    vals[0, rng.random(N) < 0.3] = np.nan
    vals[1, ::5] = np.nan
    vals[2, 1:] = np.nan                                            # one value: nothing can be tested
    genes = _edge_genes(rng, N)
    assert _check(eng, vals, genes) > 10
    got, _m = _run(eng, vals, genes, 0.95)
    assert (got["shift"][2] == 0).all() and np.isneginf(got["lower"][2]).all() and np.isposinf(got["upper"][2]).all()


def _route_sizes(lib):
    """Every N at which a block takes another number of wavefronts, and the N before it."""
    sizes, n = [], 1
    waves = lib.scoary_rank_shift_waves(1)
    while waves > 1:
        lo, hi = n, MAX_N                                           # the last N with `waves`: a bisection
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if lib.scoary_rank_shift_waves(mid) >= waves:
                lo = mid
            else:
                hi = mid - 1
        if lo == MAX_N:
            break
        sizes += [lo, lo + 1]
        n, waves = lo + 1, lib.scoary_rank_shift_waves(lo + 1)
    return sizes


def test_every_size_at_which_the_block_changes(eng):
    lib = eng.lib
    assert lib.scoary_rank_shift_waves(1) == 16 and lib.scoary_rank_shift_waves(MAX_N) == 1
    assert lib.scoary_rank_shift_waves(0) == 0 and lib.scoary_rank_shift_waves(MAX_N + 1) == 0
    sizes = _route_sizes(lib)
    assert len(sizes) == 8 and [lib.scoary_rank_shift_waves(n) for n in sizes] == [16, 8, 8, 4, 4, 2, 2, 1]
    rng = np.random.default_rng(11)
    for N in sizes:
        vals = rng.standard_normal((1, N))
        vals[0, ::7] = np.round(vals[0, ::7], 1)
        vals[0, 5::97] = np.nan
        rows = []
        for m in (1, 2, 37):
            r = np.zeros(N, bool)
            r[rng.permutation(N)[:m]] = True
            rows += [r, ~r]
        assert _check(eng, vals, np.array(rows)) >= 4


def test_heavy_ties(eng):
    rng = np.random.default_rng(300)
    vals = np.exp2(rng.integers(0, 8, (1, 300)).astype(float))      # 8 distinct values: most differences coincide
    genes = _edge_genes(rng, 300, extra=12)
    _check(eng, vals, genes, 0.95)
    got, _m = _run(eng, vals, genes, 0.95)
    assert (got["shift"][0] == 0).sum() > 3                         # ... and the median is often the zero


def test_all_distinct_values_three_traits(eng):
    rng = np.random.default_rng(333)
    vals = rng.permutation(3 * 333).reshape(3, 333) * 0.37 - 100.0
    vals[1] = rng.standard_normal(333)
    assert _check(eng, vals, _edge_genes(rng, 333, extra=10)) > 30


@pytest.mark.parametrize("G", (1, 255, 256, 257))
def test_gene_block_edges(eng, G):
    rng = np.random.default_rng(G)
    N = 33
    vals = np.stack([np.round(rng.standard_normal(N), 1), rng.standard_normal(N)])
    genes = rng.random((G, N)) < rng.uniform(0.03, 0.97, (G, 1))
    if G == 1:
        genes[0, :5] = True
        genes[0, 5:9] = False
    _check(eng, vals, genes)


def test_two_levels(eng):
    rng = np.random.default_rng(5)
    N = 50
    vals = np.stack([np.round(rng.standard_normal(N), 1), rng.standard_normal(N)])
    genes = _edge_genes(rng, N, extra=10)
    wide = _check(eng, vals, genes, 0.999, want_infinite=True)      # small genes: no interval at this level
    narrow = _check(eng, vals, genes, 0.5)
    assert narrow > wide > 0


def test_the_largest_n(eng):
    """N = 16 320: one wavefront per block; m = 8 160 has K = 66 585 600, the largest there is: past 2^25, and 2^26
    is never reached."""
    rng = np.random.default_rng(16320)
    N = MAX_N
    vals = rng.standard_normal((1, N))
    vals[0, ::3] = np.round(vals[0, ::3], 2)
    half = np.zeros(N, bool)
    half[rng.permutation(N)[:N // 2]] = True
    one = np.zeros(N, bool)
    one[N - 1] = True
    few = rng.random(N) < 0.01
    genes = np.array([half, one, ~one, few, ~few])
    assert 1 << 25 < int(half.sum()) * int((~half).sum()) == 66585600 < 1 << 26
    assert _check(eng, vals, genes, 0.95, partition=True) >= 3      # (one carrier among 16 320: no interval)


def test_a_trait_of_equal_values_and_a_plan_of_other_genes(eng):
    import torch
    rng = np.random.default_rng(3)
    N, G = 40, 9
    vals = np.stack([np.full(N, 2.5), rng.standard_normal(N)])
    genes = rng.random((G, N)) < 0.5
    got, m = _run(eng, vals, genes, 0.95)
    assert (got["shift"][0] == 0).all() and np.isneginf(got["lower"][0]).all() and (got["ca"][0] == 0).all()
    _check(eng, vals, genes)
    # m that is not the count of the gene's bits at pos: NaN, and nothing else changes
    gm = eng.pack_dense(genes.astype(np.uint8))
    plan = eng.ranksum_plan(vals)
    res = eng.ranksum(gm, plan)
    res["m"][1, 4] += 1
    out = eng.ranksum_shift(gm, plan, res)
    torch.cuda.synchronize()
    assert all(math.isnan(float(out[k][1, 4])) for k in ("shift", "lower", "upper")) and int(out["ca"][1, 4]) == 0
    keep = np.ones(G, bool)
    keep[4] = False
    assert np.array_equal(_bits(out["shift"][1].cpu().numpy()[keep]), _bits(got["shift"][1][keep]))


def test_positions_outside_the_matrix_are_clamped(eng):
    """A plan whose pos holds anything: numbers of no meaning, and no access outside the matrix -- every entry is
    clamped into [0, N).  The outputs are written for every cell."""
    import torch
    rng = np.random.default_rng(8)
    N, G = 70, 20
    vals = rng.standard_normal((1, N))
    genes = rng.random((G, N)) < 0.4
    gm = eng.pack_dense(genes.astype(np.uint8))
    plan = eng.ranksum_plan(vals)
    res = eng.ranksum(gm, plan)
    eng.ranksum_shift(gm, plan, res)
    plan.shift_plan.pos.copy_(torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31 - 1, (1, N)).astype(np.int32)))
    out = eng.ranksum_shift(gm, plan, res)
    torch.cuda.synchronize()
    shift = out["shift"].cpu().numpy()
    assert (np.isnan(shift) | np.isfinite(shift)).all()


def test_raw_entry_point_refusals(eng):
    import torch
    N, G, T = 40, 5, 1
    z = torch.zeros(4096, dtype=torch.float64, device=eng.device)
    gm = eng.pack_dense(np.zeros((G, N), dtype=np.uint8))
    p = eng._ptr(z)

    def call(tiled=None, xs=p, zq=1.96, g=G, t=T, n=N, ca=p):
        return eng.lib.scoary_ranksum_shift(eng.h, eng._ptr(gm.tiled) if tiled is None else tiled, xs, p, p, p, p,
                                            ctypes.c_double(zq), g, t, n, p, p, p, ca, eng._stream())

    assert call() == 0
    for bad in (dict(tiled=0), dict(xs=0), dict(ca=0), dict(zq=0.0), dict(zq=-1.0), dict(zq=math.inf), dict(g=0),
                dict(t=0), dict(n=0)):
        assert call(**bad) == ERR_ARG, bad
    before = z.clone()
    assert call(n=MAX_N + 1) == ERR_SIZE and call(t=65536) == ERR_SIZE
    torch.cuda.synchronize()
    assert torch.equal(z, before)
