"""k_rank_shift (spec S19) past its easy shapes, against the restatement rank_shift_spec.py bit for bit (shift, lower,
upper as uint64, ca exactly: test_gpu_rank_shift._check, with its assertion that no cell's unfloored ca is within
1e-9 of an integer -- the inputs below were chosen on the CPU so that the restatement alone satisfies it).

a. Several genes per wavefront: shapes at which the launch rule of scoary_ranksum_shift -- copied here, and fed the
   device's own CU count -- gives a trait fewer blocks than its genes need, so that a wavefront walks genes g,
   g + stride, g + 2 stride with its bit words, prefix counts and walked list written again for each: a long walked
   list before a short one and the reverse, a flipped gene before an unflipped one, untestable genes and a NaN cell
   (an m that is not the plan's) between real ones; once at sixteen wavefronts a block and once where the block has
   shrunk to eight.  The tests assert the number of rounds and that the last one is ragged.
b. The key bisection wide and narrow: subnormal values and differences, +-0.0, a bracket from key(-2e150) to
   key(2e150) (the full 64 halvings), neighbouring doubles, differences that round, a constant row but for one value.
c. Tiny traits: N = 1, and n = 0, 1 and 2 equal values next to a full trait.

(test_gpu_rank_shift.py holds the same kernel at moderate shapes, one gene per wavefront.)"""
import ctypes

import numpy as np
import pytest

import rank_shift_spec as spec
from test_gpu_rank_shift import _bits, _check, _edge_genes, _route_sizes

pytestmark = pytest.mark.gpu
DBL_MIN = 2.2250738585072014e-308
FILL = 12345.678                    # no result of these inputs
FILL_CA = -777


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.close()


# ---------------------------------------------------------------- a. several genes per wavefront ------
def _rounds(eng, G, T, N):
    """(CUs, W, blocks of a trait, stride = genes of a round, rounds) of scoary_ranksum_shift's launch on this device:
    the rule, copied."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    W = int(eng.lib.scoary_rank_shift_waves(N))
    per_trait = max(1, -(-4 * cus // T))
    nblk = min(-(-G // W), per_trait)
    return cus, W, nblk, nblk * W, -(-(-(-G // W)) // nblk)


def _gene(N, idx):
    r = np.zeros(N, bool)
    r[np.asarray(idx, dtype=int)] = True
    return r


# what one wavefront meets in rounds 0, 1, 2: carriers among the N isolates as fractions of N (0 = none, 1 = all)
_PLOTS = ((0.5, 0.03, 0.45),        # a long walked list, a short one behind whose end the long one's entries lie, long
          (0.03, 0.5, 0.06),        # ... and the reverse
          (0.9, 0.12, 0.8),         # flipped (the non-carriers walked), not flipped, flipped
          (0.3, 0.75, 0.2),         # ... and the reverse
          (0.4, 0.0, 0.55),         # no carrier between two real genes
          (0.6, 1.0, 0.35),         # every isolate a carrier between two real genes
          (0.97, 0.5, 0.0),         # one or two walked non-carriers, then a long list of carriers
          (0.0, 0.25, 1.0))


def _plotted_genes(rng, N, G, stride):
    """G genes such that slot g mod stride meets the fractions of _PLOTS[slot mod 8] in its successive rounds."""
    genes = np.zeros((G, N), bool)
    for g in range(G):
        f = _PLOTS[(g % stride) % len(_PLOTS)][(g // stride) % 3]
        genes[g] = _gene(N, rng.permutation(N)[:int(round(f * N))])
    return genes


class _Spread:
    """What test_gpu_rank_shift._run asks of an engine, for _check: the rows of ``vals`` are run as the T traits
    ``which`` names (row which[t] is trait t), every trait's outputs must equal those of the other traits with its
    row bit for bit, and _check gets the outputs of one trait per row -- ``pick[r]`` -- to hold to the restatement.
    So every one of the T x G cells is compared, at the restatement's cost of rows x G."""

    def __init__(self, eng, which, pick):
        self.eng, self.which, self.pick, self.res, self.out = eng, np.asarray(which), list(pick), None, None
        assert all(self.which[t] == r for r, t in enumerate(self.pick))

    def pack_dense(self, genes):
        return self.eng.pack_dense(genes)

    def ranksum_plan(self, vals):
        assert len(vals) == len(self.pick)
        return self.eng.ranksum_plan(np.asarray(vals)[self.which])

    def ranksum(self, gm, plan):
        self.res = self.eng.ranksum(gm, plan)
        return {k: v[self.pick] for k, v in self.res.items()}

    def ranksum_shift(self, gm, plan, _res, level=0.95):
        out = self.eng.ranksum_shift(gm, plan, self.res, level=level)
        self.out = {k: v.cpu().numpy() for k, v in out.items()}
        for t, r in enumerate(self.which):
            for k, v in self.out.items():
                assert np.array_equal(v[t].view(np.uint64), v[self.pick[r]].view(np.uint64)), (k, t, self.pick[r])
        return {k: v[self.pick] for k, v in out.items()}


def _rows_16():
    """Four rows of N = 40: ties and missing values, all distinct, MIC-like with heavy ties, distinct with few
    values."""
    rng = np.random.default_rng(4016)
    N = 40
    rows = np.stack([np.round(rng.standard_normal(N), 1), rng.standard_normal(N),
                     np.exp2(rng.integers(-2, 3, N).astype(float)), rng.standard_normal(N) * 1e3])
    rows[0, rng.permutation(N)[:6]] = np.nan
    rows[3, rng.permutation(N)[:15]] = np.nan
    return rows


def _which_16():
    rng = np.random.default_rng(64)
    which = np.concatenate([[0], rng.permutation(np.repeat(np.arange(4), 16)[1:-1]), [3]])
    pick = [int(np.flatnonzero(which == r)[-1 if r == 3 else 0]) for r in range(4)]
    assert pick[0] == 0 and pick[3] == 63 and (np.bincount(which) == 16).all()
    return which, pick


def test_three_rounds_of_genes_per_wavefront(eng):
    """N = 40 (sixteen wavefronts a block), T = 64, G = 600: on 256 CUs a trait gets 16 blocks for its 38 groups of 16
    genes, three rounds with 88 genes in the third."""
    N, T, G = 40, 64, 600
    cus, W, nblk, stride, rounds = _rounds(eng, G, T, N)
    print("CUs %d: N %d T %d G %d, W %d, %d blocks a trait, stride %d, %d rounds, %d genes in the last"
          % (cus, N, T, G, W, nblk, stride, rounds, G - (rounds - 1) * stride))
    assert W == 16 and rounds >= 3 and G % stride != 0 and G > 2 * stride
    which, pick = _which_16()
    genes = _plotted_genes(np.random.default_rng(600), N, G, stride)
    assert _check(_Spread(eng, which, pick), _rows_16(), genes) > 4 * G // 2


def test_a_nan_cell_between_two_real_ones(eng):
    """The raw entry point over the shape above into prefilled outputs, twice: as it is, and with m of a few
    middle-round cells raised by one.  Those cells become (NaN, NaN, NaN, 0), their wavefront's genes before and
    behind them are real ones, and no other cell changes."""
    import torch
    N, T, G = 40, 64, 600
    _cus, _W, _nblk, stride, rounds = _rounds(eng, G, T, N)
    assert rounds >= 3 and G > 2 * stride
    which, _pick = _which_16()
    vals = _rows_16()[which]
    genes = _plotted_genes(np.random.default_rng(600), N, G, stride)
    gm = eng.pack_dense(genes.astype(np.uint8))
    plan = eng.ranksum_plan(vals)
    res = eng.ranksum(gm, plan)
    eng.ranksum_shift(gm, plan, res)                                 # (makes plan.shift_plan)
    var = eng.ranksum_var(plan, res["m"])
    zq = spec.zq_of(0.95)

    def launch(m):
        out = {k: torch.full((T, G), FILL, dtype=torch.float64, device=eng.device) for k in ("shift", "lower", "upper")}
        out["ca"] = torch.full((T, G), FILL_CA, dtype=torch.int64, device=eng.device)
        eng._check(eng.lib.scoary_ranksum_shift(
            eng.h, eng._ptr(gm.tiled), eng._ptr(plan.shift_plan.xs), eng._ptr(plan.shift_plan.pos),
            eng._ptr(plan.valid), eng._ptr(m), eng._ptr(var), ctypes.c_double(zq), G, T, N,
            *(eng._ptr(out[k]) for k in ("shift", "lower", "upper", "ca")), eng._stream()), "scoary_ranksum_shift")
        return {k: v.cpu().numpy() for k, v in out.items()}

    base = launch(res["m"])
    assert all((_bits(base[k]) != _bits(FILL)).all() for k in ("shift", "lower", "upper")) and (base["ca"] != FILL_CA).all()
    real = np.isfinite(base["lower"])                                # cells with limits: tested genes
    cells = [(t, g) for t in (0, 17, 63) for g in range(stride, stride + G - 2 * stride)
             if real[t, g - stride] and real[t, g] and real[t, g + stride]][::7]
    assert len(cells) >= 6
    m = res["m"].clone()
    for t, g in cells:
        m[t, g] += 1
    got = launch(m)
    hit = np.zeros((T, G), bool)
    hit[tuple(np.array(cells).T)] = True
    for k in ("shift", "lower", "upper"):
        assert np.isnan(got[k][hit]).all(), k
        assert np.array_equal(_bits(got[k])[~hit], _bits(base[k])[~hit]), k
    assert (got["ca"][hit] == 0).all() and np.array_equal(got["ca"][~hit], base["ca"][~hit])


def test_four_rounds_where_the_block_has_eight_wavefronts(eng):
    """The smallest N at which a block has eight wavefronts, T = 1024 (two rows, 512 times each), so that a trait has
    one block on any device with at most 256 CUs, and G = 3 W + 1: four rounds, one gene in the last."""
    N = _route_sizes(eng.lib)[1]
    T, G = 1024, 25
    cus, W, nblk, stride, rounds = _rounds(eng, G, T, N)
    print("CUs %d: N %d T %d G %d, W %d, %d blocks a trait, stride %d, %d rounds, %d genes in the last"
          % (cus, N, T, G, W, nblk, stride, rounds, G - (rounds - 1) * stride))
    assert W == 8 and eng.lib.scoary_rank_shift_waves(N - 1) == 16 and G == 3 * W + 1
    assert nblk == 1 and rounds >= 3 and G % stride != 0
    rng = np.random.default_rng(N)
    rows = np.stack([rng.standard_normal(N), np.round(rng.standard_normal(N), 2)])
    rows[0, rng.random(N) < 0.1] = np.nan
    which = np.concatenate([[0], rng.permutation(np.repeat([0, 1], T // 2)[1:-1]), [1]])
    pick = [0, T - 1]
    # what wavefront w meets in its rounds: a fraction of the isolates, or their number (0 = none, N = all); the last
    # entry is wavefront 0's alone.  K is small in most cells: the restatement partitions K differences for each
    plots = ((0.5, 3, 0, 0.004), (2, 0.3, N, 0), (N - 3, 0.01, 40, 0), (0.02, N - 1, 0.4, 0),
             (1, N - 40, 5, 0), (0.45, 0, N - 2, 0), (N, 60, 0.97, 0), (0, 0.2, 1, 0))
    genes = np.zeros((G, N), bool)
    for g in range(G):
        f = plots[g % W][g // W]
        genes[g] = _gene(N, rng.permutation(N)[:int(f if f >= 1 or f == 0 else round(f * N))])
    assert _check(_Spread(eng, which, pick), rows, genes, partition=True) > G


# ---------------------------------------------------------------- b. wide and narrow key ranges ------
def _families():
    """Five rows of N = 32: the value families of test_rank_shift_spec.py and three more."""
    rng = np.random.default_rng(1907)
    N = 32
    tiny = np.concatenate([rng.integers(-6, 7, 18) * 5e-324, rng.standard_normal(10) * 1e-310, [-0.0, 0.0, -0.0, 0.0]])
    # (twelve normals below zero and twelve above: the isolate with 5e-324 against all others has the median 5e-324)
    normals = np.abs(rng.standard_normal(N - 8)) * np.repeat([-1.0, 1.0], (N - 8) // 2)
    wide = np.concatenate([[-1e150, -2.5, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1e150], normals])
    ulps = 1.0 + rng.permutation(64)[:N] * 2.0 ** -52                # exact differences of a few ulps of 1
    # +-(1e16 + 2 k) next to 0 .. 9: the sum or difference of a large and a small one rounds to a multiple of 2
    big = np.concatenate([1e16 + 2.0 * rng.permutation(12)[:11], -1e16 - 2.0 * rng.permutation(12)[:11],
                          rng.integers(0, 10, 10).astype(float)])
    const = np.full(N, 7.25)
    const[11] = -3.0
    rows = np.stack([tiny, wide, ulps, big, const])
    assert rows.shape == (5, N)
    return rows


def _family_genes(N):
    """_edge_genes and, with their complements: the isolates of -5e-324 and of 5e-324 of the second row alone, and the
    one value of the constant row alone."""
    genes = _edge_genes(np.random.default_rng(32), N, extra=10)
    alone = np.array([_gene(N, [2]), _gene(N, [5]), _gene(N, [11])])
    return np.concatenate([genes, alone, ~alone])


def test_wide_and_narrow_key_ranges(eng):
    rows = _families()
    N = rows.shape[1]
    genes = _family_genes(N)
    assert spec.key_of(float(rows[1].max() - rows[1].min())) - spec.key_of(float(rows[1].min() - rows[1].max())) \
        > 2 ** 63                                                    # the bracket takes the full 64 halvings
    x = rows[3][:, None] - rows[3][None, :]
    assert (np.abs(x) > 2.0 ** 53).any() and (x % 2 == 0)[np.abs(x) > 2.0 ** 53].all() and (rows[3] % 2 == 1).any()
    assert _check(eng, rows, genes) > 3 * len(genes)
    # _check has held every cell to the restatement bit for bit; what the restatement's values are
    plus_zero, subnormal = _zeros_and_subnormals(rows, genes)
    print("cells whose median difference is a zero: %s; subnormal results: %s" % (plus_zero, subnormal))
    assert plus_zero[0] > 0 and plus_zero[4] > 0
    assert subnormal[0] > len(genes) and subnormal[1] > 0 and not any(subnormal[2:])


def _zeros_and_subnormals(rows, genes):
    """Per row: the tested cells whose median difference (numpy's) is a zero -- their shift is +0.0, asserted -- and
    the results (shift, lower, upper) that are subnormal, both by the restatement."""
    plus_zero, subnormal = [0] * len(rows), [0] * len(rows)
    for t, row in enumerate(rows):
        for gene in genes:
            shift, lower, upper, _ca, _raw = spec.shift_spec(row, gene)
            a, b, x = spec.split(row, gene)
            if spec.s15_var(x, a.size) > 0 and np.median(np.subtract.outer(a, b)) == 0:
                assert _bits(shift) == 0                             # the sign bit clear
                plus_zero[t] += 1
            subnormal[t] += sum(0.0 < abs(v) < DBL_MIN for v in (shift, lower, upper))
    return plus_zero, subnormal


# ---------------------------------------------------------------- c. tiny traits ------
def _untestable(out, t):
    return ((_bits(out["shift"][t]) == 0).all() and np.isneginf(out["lower"][t]).all()
            and np.isposinf(out["upper"][t]).all() and (out["ca"][t] == 0).all())


def _outputs(eng, vals, genes):
    gm = eng.pack_dense(np.ascontiguousarray(genes, dtype=np.uint8))
    plan = eng.ranksum_plan(vals)
    return {k: v.cpu().numpy() for k, v in eng.ranksum_shift(gm, plan, eng.ranksum(gm, plan)).items()}


def test_one_isolate(eng):
    vals = np.array([[4.0], [np.nan]])
    genes = np.array([[0], [1]], dtype=bool)
    _check(eng, vals, genes, want_infinite=True)
    out = _outputs(eng, vals, genes)
    assert out["shift"].shape == (2, 2) and _untestable(out, 0) and _untestable(out, 1)


@pytest.mark.parametrize("N", (33, 64))
def test_traits_of_zero_one_and_two_equal_values_next_to_a_full_one(eng, N):
    rng = np.random.default_rng(N)
    full = np.round(rng.standard_normal(N), 1)
    vals = np.full((6, N), np.nan)
    vals[0] = full
    vals[2, N - 1] = 1.5                                             # n = 1, the last isolate
    vals[3] = full
    vals[4, [3, N - 2]] = -2.25                                      # n = 2, equal: every valid value tied
    vals[5, [0, N - 1]] = [1.0, 3.0]                                 # n = 2, distinct: m = 1 is a real gene
    genes = _edge_genes(rng, N)
    genes = np.concatenate([genes, [_gene(N, [0]), _gene(N, [N - 1]), _gene(N, [3]), _gene(N, [3, N - 2])]])
    assert _check(eng, vals, genes) > len(genes)
    out = _outputs(eng, vals, genes)
    assert all(_untestable(out, t) for t in (1, 2, 4)) and not _untestable(out, 5)
    alone = _outputs(eng, vals[:1], genes)                           # the full trait without its neighbours
    for t in (0, 3):
        assert all(np.array_equal(_bits(out[k][t]), _bits(alone[k][0])) for k in ("shift", "lower", "upper"))
        assert np.array_equal(out["ca"][t], alone["ca"][0]) and not _untestable(out, t)
