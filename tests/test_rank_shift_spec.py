"""Spec S19 (the Hodges-Lehmann shift of the rank-sum test and its confidence limits) on the CPU: the restatement
rank_shift_spec.py against numpy.median, its two statements of an order statistic against each other, ca on
hand-worked cases, the symmetries, and the coverage of the interval.  No GPU."""
import math

import numpy as np
import pytest

import rank_shift_spec as spec


def _cases():
    rng = np.random.default_rng(1907)
    mic = np.exp2(rng.integers(-3, 5, 40).astype(float))                      # MIC-like: heavy ties
    normal = rng.standard_normal(37)                                          # all distinct
    tiny = np.concatenate([rng.integers(-6, 7, 12) * 5e-324, rng.standard_normal(9) * 1e-310, [-0.0, 0.0, -2.5, 3.0]])
    out = []
    for name, x in (("mic", mic), ("normal", normal), ("subnormal", tiny)):
        n = x.size
        for m in (1, 2, 3, n // 2, n - 2, n - 1):                             # K odd and even among them
            bits = np.zeros(n, dtype=bool)
            bits[rng.permutation(n)[:m]] = True
            out.append(("%s-m%d" % (name, m), x, bits))
    return out


CASES = _cases()


def test_the_cases_have_odd_and_even_k():
    ks = {int(bits.sum()) * int((~bits).sum()) % 2 for _name, _x, bits in CASES}
    assert ks == {0, 1}


@pytest.mark.parametrize("name,x,bits", CASES, ids=[c[0] for c in CASES])
def test_shift_is_numpy_median_to_the_bit(name, x, bits):
    a, b, _all = spec.split(x, bits)
    want = np.median(np.subtract.outer(a, b))
    shift, lower, upper, ca, _raw = spec.shift_spec(x, bits)
    assert np.float64(shift).tobytes() == np.float64(want + 0.0).tobytes()
    assert lower <= shift <= upper
    assert ca <= a.size * b.size // 2
    if shift == 0:
        assert math.copysign(1.0, shift) == 1.0


def test_bisection_is_brute_force_at_every_rank():
    rng = np.random.default_rng(5)
    for x in (np.exp2(rng.integers(-2, 3, 9).astype(float)), rng.standard_normal(8),
              np.concatenate([rng.integers(-3, 4, 5) * 5e-324, [0.0, -1.5, 1e-308]])):
        for m in (1, 3, x.size - 1):
            a, b = x[:m] + 0.0, x[m:] + 0.0
            d = spec.differences(a, b)
            for rank in range(1, d.size + 1):
                got = spec.select_by_bisection(a, b, rank)
                assert np.float64(got).tobytes() == np.float64(spec.order_statistic(d, rank)).tobytes(), (m, rank)


def test_keys_keep_the_order_of_the_doubles():
    v = [-1e150, -2.5, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1e150]
    keys = [spec.key_of(x) for x in v]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert all(np.float64(spec.value_of(spec.key_of(x))).tobytes() == np.float64(x).tobytes() for x in v)


def test_ca_on_hand_worked_cases():
    zq = spec.zq_of(0.95)
    assert abs(zq - 1.959963984540054) < 1e-12
    # n = 4, m = 2, no ties: K = 4, var = (4 / 12) * 5 = 5 / 3, 2 - 1.96 * 1.291 = -0.53: no interval at 95 %
    x = np.array([1.0, 2.0, 3.0, 4.0])
    bits = np.array([1, 0, 1, 0])
    assert spec.s15_var(x, 2) == (4.0 / 12.0) * 5.0
    shift, lower, upper, ca, raw = spec.shift_spec(x, bits)
    assert ca == -1 and -0.54 < raw < -0.52 and (lower, upper) == (-math.inf, math.inf)
    assert shift == -1.0                                 # differences -3, -1, -1, 1
    # n = 10, m = 5, no ties: K = 25, var = (25 / 12) * 11, 12.5 - 1.96 * 4.787 = 3.117: ca = 3, d_(3) and d_(23)
    x = np.arange(10, dtype=float)
    bits = np.array([0, 0, 0, 1, 0, 1, 1, 0, 1, 1])
    shift, lower, upper, ca, raw = spec.shift_spec(x, bits)
    d = spec.differences(x[bits == 1], x[bits == 0])
    assert ca == 3 and 3.11 < raw < 3.12 and (lower, upper) == (d[2], d[22]) and shift == d[12]
    # the same at 50 %: zq = 0.674, 12.5 - 3.229 = 9.27: ca = 9
    assert spec.shift_spec(x, bits, level=0.5)[3] == 9
    # ties lower the variance: n = 6 with two groups of three, tiesum 48, f = 7 - 48 / 30 = 5.4
    x = np.array([1.0, 1.0, 1.0, 2.0, 2.0, 2.0])
    assert spec.s15_var(x, 2) == (8.0 / 12.0) * (7.0 - 48.0 / 30.0)
    # untestable: all values tied (f = 0), m = 0, m = n
    assert spec.shift_spec(np.ones(5), [1, 0, 1, 0, 0])[:4] == (0.0, -math.inf, math.inf, 0)
    assert spec.shift_spec(x, np.zeros(6))[:4] == (0.0, -math.inf, math.inf, 0)
    assert spec.shift_spec(x, np.ones(6))[:4] == (0.0, -math.inf, math.inf, 0)


def test_missing_values_leave_the_sets():
    x = np.array([1.0, np.nan, 3.0, 4.0, np.nan, 8.0])
    bits = np.array([1, 1, 0, 1, 0, 0])
    a, b, v = spec.split(x, bits)
    assert a.tolist() == [1.0, 4.0] and b.tolist() == [3.0, 8.0] and v.size == 4
    with pytest.raises(ValueError):
        spec.split(np.array([1.0, 2e150]), [1, 0])


def test_complement_antisymmetry_and_translation():
    rng = np.random.default_rng(77)
    for trial in range(40):
        n = int(rng.integers(5, 30))
        x = rng.integers(-50, 51, n).astype(float) if trial % 2 else rng.standard_normal(n)
        bits = rng.random(n) < 0.4
        if bits.sum() in (0, n):
            bits[0] = ~bits[0]
        for level in (0.5, 0.95):
            s, lo, up, ca, _ = spec.shift_spec(x, bits, level)
            s2, lo2, up2, ca2, _ = spec.shift_spec(x, ~bits, level)
            assert (s2, lo2, up2, ca2) == (-s + 0.0, -up + 0.0, -lo + 0.0, ca)
            if trial % 2:                                # integer-valued data: every sum is exact
                # (the pooled ties, and with them var and ca, change with delta: the order statistics translate, so
                # the limits do at the same ca)
                delta = float(rng.integers(-1000, 1000))
                s3, lo3, up3, ca3, _ = spec.shift_spec(np.where(bits, x + delta, x), bits, level, ca=ca)
                assert (s3, lo3, up3, ca3) == (s + delta, lo + delta, up + delta, ca)


def test_the_interval_covers_the_true_shift():
    """2 000 draws of two normal samples (12 carriers, 15 non-carriers, true shift 1.0) at L = 0.95: the share of
    intervals that hold 1.0 is not below 0.95 - 3 sqrt(0.95 * 0.05 / 2000) = 0.935."""
    rng = np.random.default_rng(20261020)
    bits = np.arange(27) < 12
    covered = 0
    for _ in range(2000):
        x = rng.standard_normal(27)
        x[:12] += 1.0
        _s, lower, upper, ca, _ = spec.shift_spec(x, bits)
        assert ca >= 1
        covered += lower <= 1.0 <= upper
    assert covered / 2000.0 >= 0.95 - 3.0 * math.sqrt(0.95 * 0.05 / 2000.0)
