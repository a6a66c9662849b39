"""Spec S9 (labels shuffled within strata), host only: the plain-Python restatement (strata_spec.py) against S4
for one stratum, its per-stratum margins, and the law itself on a small case."""
import itertools

import numpy as np

from oracle import oracle as orc
from strata_spec import s9_labels
from test_gpu_strata import _spec_case

SEED = 0x0123456789ABCDEF


def _s4(seed, t, pi, valid, npos):
    N = len(valid)
    mb = orc.pack_rows(np.asarray(valid, dtype=np.uint8)[None])[0]
    return np.unpackbits(orc.perm_labels(seed, t, pi, mb, npos, N).view(np.uint8), bitorder="little")[:N].tolist()


def _observed(valid, npos):
    """Some observed labelling with npos positives on the valid isolates (S9 reads only its per-stratum counts)."""
    lab, left = [0] * len(valid), npos
    for i, v in enumerate(valid):
        if v and left > 0:
            lab[i], left = 1, left - 1
    return lab


def test_one_stratum_is_spec_s4_every_margin_of_small_n():
    for N in range(1, 10):
        for missing in (0, 1, 2):
            if missing >= N:
                continue
            valid = [1] * N
            for k in range(missing):
                valid[(3 * k + 1) % N] = 0
            nval = sum(valid)
            for npos in range(nval + 1):
                lab = _observed(valid, npos)
                for t, pi in ((0, 0), (2, 37), (65535, 4_000_000_123)):
                    assert s9_labels(SEED, t, pi, valid, lab, [0] * N) == _s4(SEED, t, pi, valid, npos), \
                        (N, missing, npos, t, pi)


def test_one_stratum_is_spec_s4_word_boundaries_with_missing_values():
    rng = np.random.default_rng(9)
    for N in (63, 64, 65, 257):
        valid = (rng.random(N) >= 0.15).astype(int).tolist()
        valid[0] = 1
        nval = sum(valid)
        for npos in sorted({0, 1, nval // 7, nval // 2, nval // 2 + 1, nval - 1, nval}):
            lab = _observed(valid, npos)
            for t, pi in ((1, 5), (3, 64), (9, 1_000_003)):
                assert s9_labels(SEED, t, pi, valid, lab, [0] * N) == _s4(SEED, t, pi, valid, npos), (N, npos, t, pi)


def test_every_stratum_keeps_its_positives():
    rng = np.random.default_rng(4)
    for N, S in ((40, 3), (97, 7), (130, 16)):
        strata = rng.integers(0, S, N).tolist()
        strata[:S] = range(S)                        # interleaved, none empty
        valid = (rng.random(N) >= 0.1).astype(int).tolist()
        lab = [int(v and rng.random() < 0.4) for v in valid]
        want = [sum(lab[i] for i in range(N) if strata[i] == s) for s in range(S)]
        for pi in (0, 1, 31, 32, 1000, 77_777):
            got = s9_labels(SEED, 2, pi, valid, lab, strata, S)
            assert [sum(got[i] for i in range(N) if strata[i] == s) for s in range(S)] == want, (N, S, pi)
            assert not any(g and not v for g, v in zip(got, valid))
    # a stratum without valid members, a stratum that is all positive, an empty stratum (S given)
    strata = [0, 1, 0, 1, 2, 2, 0, 4]
    valid = [1, 0, 1, 0, 1, 1, 1, 1]
    lab = [1, 0, 0, 0, 1, 1, 0, 0]
    for pi in range(40):
        got = s9_labels(SEED, 0, pi, valid, lab, strata, 5)
        assert got[1] == got[3] == 0 and got[4] == got[5] == 1 and got[7] == 0
        assert got[0] + got[2] + got[6] == 1


def test_the_law_is_uniform_and_independent_across_strata():
    """N = 11; stratum A = {0, 2, 4, 9} with 2 positives (6 subsets), stratum B = the other 7 isolates, one of them
    missing, 3 positives (20 subsets): the 120 joint outcomes are equally likely.  P = 48 000 permutations at seed
    1, 400 expected per outcome; chi-square on 119 degrees of freedom below 119 + 5 sqrt(238) ~ 196.
    (Value at seed 1: 107.31.  The seed is not searched: a failure here is a defect of the spec.)"""
    N, P = 11, 48_000
    A = [0, 2, 4, 9]
    Bm = [i for i in range(N) if i not in A]
    strata = [0 if i in A else 1 for i in range(N)]
    valid = [1] * N
    valid[Bm[3]] = 0
    Bv = [i for i in Bm if valid[i]]
    lab = [0] * N
    lab[A[0]] = lab[A[1]] = 1
    lab[Bv[0]] = lab[Bv[1]] = lab[Bv[2]] = 1
    outcomes = {(a, b): 0 for a in itertools.combinations(A, 2) for b in itertools.combinations(Bv, 3)}
    assert len(outcomes) == 120
    for pi in range(P):
        got = s9_labels(1, 0, pi, valid, lab, strata)
        key = (tuple(i for i in A if got[i]), tuple(i for i in Bv if got[i]))
        assert sum(got) == 5 and not got[Bm[3]]
        outcomes[key] += 1
    exp = P / 120.0
    chi2 = sum((c - exp) ** 2 / exp for c in outcomes.values())
    print("chi2 = %.2f on 119 degrees of freedom" % chi2)
    assert chi2 < 119 + 5 * (2 * 119) ** 0.5


def test_the_multipass_case_has_small_and_batched_fix_ups_past_the_first_pass():
    """The case test_gpu_strata.py compares with this restatement: strata of every size class, and among the
    checked permutations strata with index >= 32 (a block's second and third pass over the strata at 32 lanes per
    permutation) whose fix-up starts 4 or more marks off its target, and others 1 to 3 off."""
    N, P, strata, traits, perms = _spec_case("n5000_three_passes")
    S = 70
    sizes = np.bincount(strata, minlength=S)
    assert N == 5000 and traits.shape == (2, N) and (traits[0] == 2).any() and not (traits[1] == 2).any()
    assert (sizes > 0).sum() == 60 and ((sizes > 0) & (sizes <= 3)).sum() == 6 and (sizes > 300).sum() == 2
    assert ((sizes >= 40) & (sizes <= 120)).sum() == 52 and sizes[64:].any() and sizes[32:64].any()
    assert (np.diff(strata) != 0).mean() > 0.9                       # interleaved
    assert set(perms) == {0, 1, 31, 32, 33, P - 1}
    valid, lab = (traits != 2).astype(int), (traits == 1).astype(int)
    big, small = set(), set()
    for t in range(2):
        for pi in perms:
            d = {}
            got = s9_labels(0xDEADBEEF12345678, 3 + t, pi, valid[t].tolist(), lab[t].tolist(), strata.tolist(), S,
                            deficits=d)
            assert sorted(d) == np.flatnonzero(sizes).tolist()
            assert np.array_equal(np.bincount(strata, weights=got, minlength=S),
                                  np.bincount(strata, weights=lab[t], minlength=S))
            big |= {s for s, v in d.items() if s >= 32 and abs(v) >= 4}
            small |= {s for s, v in d.items() if s >= 32 and 0 < abs(v) < 4}
    print("strata >= 32 with |d| >= 4: %d, with 0 < |d| < 4: %d" % (len(big), len(small)))
    assert any(s >= 64 for s in big) and any(32 <= s < 64 for s in big)
    assert any(s >= 64 for s in small) and any(32 <= s < 64 for s in small)
