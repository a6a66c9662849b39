"""Spec S15 (the rank-sum test of a quantitative trait), host only: the plain-Python restatement (ranksum_spec.py)
against scipy.stats.mannwhitneyu, its untestable branch, the digit split, the law of the value shuffle on a small
case, the composition of batches, and the engine's host ranking against the restatement's."""
import itertools
import math

import numpy as np
import pytest
from scipy import stats

import ranksum_spec as rs
from scoary_amd.engine import rank_rows


def _cases():
    """(name, values [N] with nan for missing, gene rows) -- the gene rows of every case end with one gene on a
    single valid isolate and one on all valid isolates but one (m = 1 and m = n - 1)."""
    rng = np.random.default_rng(15)
    out = []
    for name, N, draw, missing in (("ties", 40, lambda n: rng.integers(0, 6, n).astype(float), 0.0),
                                   ("distinct", 57, lambda n: rng.permutation(n) * 0.37 - 3.0, 0.0),
                                   ("missing", 64, lambda n: rng.integers(0, 6, n).astype(float), 0.2),
                                   ("missing-distinct", 33, lambda n: rng.standard_normal(n), 0.3)):
        x = draw(N)
        x[rng.random(N) < missing] = np.nan
        genes = (rng.random((12, N)) < rng.uniform(0.1, 0.9, (12, 1))).astype(int)
        val = np.flatnonzero(~np.isnan(x))
        one = np.zeros(N, dtype=int)
        one[val[3]] = 1
        but_one = (~np.isnan(x)).astype(int)
        but_one[val[5]] = 0
        out.append((name, x.tolist(), genes.tolist() + [one.tolist(), but_one.tolist()]))
    return out


@pytest.mark.parametrize("name,x,genes", _cases(), ids=[c[0] for c in _cases()])
def test_p_and_auc_are_scipys_mannwhitneyu(name, x, genes):
    valid, rc, n, tiesum, _ = rs.ranks(x)
    ms = set()
    for gene in genes:
        D, m = rs.statistic(gene, valid, rc)
        ok, auc, p = rs.tail(D, m, n, tiesum)
        assert ok and 0 < m < n
        ms.add(m)
        a = [x[i] for i in range(len(x)) if valid[i] and gene[i]]
        b = [x[i] for i in range(len(x)) if valid[i] and not gene[i]]
        ref = stats.mannwhitneyu(a, b, use_continuity=True, alternative="two-sided", method="asymptotic")
        assert math.isfinite(ref.pvalue) and math.isfinite(ref.statistic)
        assert abs(p - ref.pvalue) <= 1e-12 * ref.pvalue, (name, m, p, ref.pvalue)
        # 0.5 + D / (2 m (n - m)) rounds twice, U / (m (n - m)) once, both are at most 1: three half-ulps of 1 apart
        # at the most (equal in the real numbers: U = D / 2 + m (n - m) / 2)
        assert abs(auc - ref.statistic / (m * (n - m))) <= 3 * 2.0 ** -53, (name, m)
        assert 2 * ref.statistic == D + m * (n - m)
    assert {1, n - 1} <= ms


def test_untestable_genes_take_their_branch():
    valid, rc, n, tiesum, groups = rs.ranks([2.5] * 9 + [math.nan])
    assert n == 9 and groups == 1 and tiesum == 9 ** 3 - 9 and rc == [0] * 10
    gene = [1, 0, 1, 1, 0, 0, 0, 1, 0, 1]
    D, m = rs.statistic(gene, valid, rc)
    assert (D, m) == (0, 4) and rs.tail(D, m, n, tiesum) == (False, 0.5, 1.0)       # every value tied: f = 0
    valid, rc, n, tiesum, _ = rs.ranks([1.0, 2.0, math.nan, 2.0, 7.0])
    for gene in ([0, 0, 1, 0, 0], [1, 1, 0, 1, 1], [1, 1, 1, 1, 1]):                # m = 0, m = n, m = n
        D, m = rs.statistic(gene, valid, rc)
        assert D == 0 and m in (0, n) and rs.tail(D, m, n, tiesum) == (False, 0.5, 1.0)
    valid, rc, n, tiesum, _ = rs.ranks([math.nan, 4.0])                             # n = 1
    assert rc == [0, 0] and rs.tail(0, 1, 1, 0) == (False, 0.5, 1.0)
    assert rs.tail(0, 0, 0, 0) == (False, 0.5, 1.0)


def test_digits_recompose_every_rank_of_the_largest_matrix():
    n = rs.MAX_ISOLATES
    for rc in range(-(n - 1), n):
        hi, lo = rs.digits(rc)
        assert 128 * hi + lo == rc and -64 <= lo <= 63 and -128 <= hi <= 127, rc
    assert rs.digits(n - 1) == (127, 63) and rs.digits(n)[0] == 128                 # the limit is sharp


def test_host_ranking_is_the_restatements():
    rng = np.random.default_rng(3)
    vals = np.stack([rng.integers(0, 6, 90).astype(float), rng.standard_normal(90), np.full(90, 1.5),
                     np.round(rng.standard_normal(90), 1)])
    vals[0, ::7] = np.nan
    vals[3, 5:60] = np.nan
    vals[2, 1:] = np.nan                                                            # n = 1
    rc, valid, n, tiesum, groups = rank_rows(vals)
    for t in range(4):
        want = rs.ranks(vals[t].tolist())
        assert (valid[t].astype(int).tolist(), rc[t].tolist(), int(n[t]), int(tiesum[t]), int(groups[t])) == want
        assert rc[t].sum() == 0


def test_the_law_of_the_value_shuffle_is_uniform():
    """n = 5 valid isolates of 6 with distinct values: the 120 orders of the permuted row are equally likely.
    P = 24 000 permutations at seed 1, 200 expected per order; chi-square on 119 degrees of freedom below
    119 + 5 sqrt(238) ~ 196, the margin of the S9 law test.  (The seed is not searched.)"""
    x = [0.5, 3.0, math.nan, -1.0, 8.0, 2.0]
    valid, rc, n, tiesum, _ = rs.ranks(x)
    assert sorted(r for r, v in zip(rc, valid) if v) == [-4, -2, 0, 2, 4]
    P = 24_000
    outcomes = {o: 0 for o in itertools.permutations([-4, -2, 0, 2, 4])}
    for pi in range(P):
        row = rs.perm_row(1, 0, pi, valid, rc)
        assert row[2] == 0
        outcomes[tuple(r for r, v in zip(row, valid) if v)] += 1
    exp = P / 120.0
    chi2 = sum((c - exp) ** 2 / exp for c in outcomes.values())
    print("chi2 = %.2f on 119 degrees of freedom" % chi2)
    assert chi2 < 119 + 5 * (2 * 119) ** 0.5


def test_r_q_composes_over_batches_and_rows_are_functions_of_seed_trait_permutation():
    rng = np.random.default_rng(8)
    N, G, P = 30, 9, 40
    x = rng.integers(0, 4, N).astype(float)
    x[[4, 17]] = np.nan
    valid, rc, n, tiesum, _ = rs.ranks(x.tolist())
    genes = (rng.random((G, N)) < 0.4).astype(int).tolist()
    genes[0] = [0] * N
    d_obs = [rs.statistic(g, valid, rc)[0] for g in genes]
    rows = [rs.perm_row(77, 1, pi, valid, rc) for pi in range(P)]
    for row in rows:
        assert sorted(row) == sorted(rc) and all(r == 0 for r, v in zip(row, valid) if not v)
    assert rows[3] != rows[4] and rs.perm_row(77, 2, 3, valid, rc) != rows[3] != rs.perm_row(78, 1, 3, valid, rc)
    whole = rs.r_q(genes, rows, d_obs)
    a, b = rs.r_q(genes, rows[:13], d_obs), rs.r_q(genes, rows[13:], d_obs)
    assert whole == [u + v for u, v in zip(a, b)]
    assert whole[0] == P                                                            # untestable: r = P
    assert max(whole) <= P and any(0 < r < P for r in whole[1:])


@pytest.mark.parametrize("N", (1, 33, 256, 257))
def test_b_operand_decodes_to_what_was_encoded(N):
    """bfrag_encode / bfrag_decode, the byte order of include/scoary_hip.h in numpy: a round trip over random rows
    with |Rc| up to 16 319, the size formula, and single entries at byte offsets worked out by hand from the
    header's sentence (so that a transposition the two functions share would show)."""
    rng = np.random.default_rng(N)
    T, P = 3, 70
    rows = rng.integers(-16319, 16320, (T, P, N))
    rows[0, 0, :] = 16319
    rows[1, P - 1, :] = -16319
    buf = rs.bfrag_encode(rows, N)
    chunks = (N + 255) // 256
    assert buf.dtype == np.uint8 and buf.size == T * ((P + 63) // 64) * chunks * 32768 == rs.bfrag_bytes(N, P, T)
    got, dig, pad, past = rs.bfrag_decode(buf, T, P, N)
    assert np.array_equal(got, rows)
    assert dig.shape == (T, P, N, 2) and pad.shape == (T, P, 256 * chunks - N, 2)
    assert past.shape == (T, 128 - P, 256 * chunks, 2) and not pad.any() and not past.any()
    for t, p, i in ((0, 0, 0), (2, 69, N - 1), (1, 31, N // 2), (1, 32, N - 1), (2, 63, 0), (0, 64, N // 3)):
        hi, lo = rs.digits(int(rows[t, p, i]))
        assert (int(dig[t, p, i, 0]), int(dig[t, p, i, 1])) == (hi, lo)
        stage, tile, lane = p // 64, (p % 64) // 32, p % 32 + 32 * ((i % 32) // 16)
        at = ((t * 2 + stage) * 8 * chunks + i // 32) * 4096 + tile * 1024 + lane * 16 + i % 16
        assert buf[at] == hi % 256 and buf[at + 2048] == lo % 256, (t, p, i)
    with pytest.raises(AssertionError):
        rs.bfrag_encode(np.full((1, 1, N), 16320), N)
