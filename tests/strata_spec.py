"""Spec S9 for ONE (seed, trait, permutation), in plain Python: labels shuffled within
strata.  A helper, not a test; written from the specification, independently of the kernel, on top of the
oracle's Philox block function and S4 plan only (the shape of the S4 restatement in test_oracle_golden.py)."""
import functools

from oracle import oracle as orc

DOM_BERN_LO, DOM_BERN_HI, DOM_FIX = 0x53434F42, 0x53434F43, 0x53434F44      # "SCOB", "SCOC", "SCOD"
FIX_MAX_CALLS = 1 << 20


@functools.lru_cache(maxsize=1 << 16)
def _philox_cached(ctr, key):
    return tuple(int(x) for x in orc.philox4x32_10(ctr, key))


def _philox(ctr, key):
    # (the round-0 words are shared by the 32 permutations of a block: a caller that walks permutations in order
    # gets them from the cache)
    return list(_philox_cached(tuple(ctr), tuple(key)))


def s9_labels(seed, t, pi, valid, labels, strata, S=None, deficits=None):
    """The 0/1 labels of permutation ``pi`` of trait ``t``: ``valid`` / ``labels`` / ``strata`` are N-long
    sequences (validity 0/1, observed label 0/1, stratum index in [0, S)).  ``deficits``: a dict that receives
    {stratum: d}, the marks every non-empty stratum's fix-up starts short of (d > 0) or past (d < 0) its target."""
    N = len(valid)
    if S is None:
        S = max(strata) + 1
    key = [seed & 0xffffffff, seed >> 32]
    B, bit = pi >> 5, pi & 31
    members = [[] for _ in range(S)]
    for i in range(N):                                  # ascending index order within every stratum
        members[strata[i]].append(i)
    out = [0] * N
    for s in range(S):
        mem = members[s]
        n_s = len(mem)
        if n_s == 0:
            continue
        nval = sum(1 for i in mem if valid[i])
        npos = sum(1 for i in mem if valid[i] and labels[i])
        m, flip, q = orc.perm_plan(npos, nval)
        # round 0: S4's bern_word of the isolate, with the stratum's q
        marks = {}
        for i in mem:
            x = 0
            if valid[i] and q:
                R = _philox([i, B, t, DOM_BERN_LO], key) + _philox([i, B, t, DOM_BERN_HI], key)
                for j in range(8):
                    x = (x | R[j]) if (q >> j) & 1 else (x & R[j])
            marks[i] = (x >> bit) & 1
        # fix-up: draws c = 0, 1, ... from counter ((s << 20) | (c >> 2), pi, t, "SCOD"), word c & 3
        d = m - sum(marks[i] for i in mem if valid[i])
        if deficits is not None:
            deficits[s] = d
        thr = (1 << 32) % n_s
        c, rnd = 0, None
        while d != 0:
            if c % 4 == 0:
                assert (c >> 2) < FIX_MAX_CALLS
                rnd = _philox([(s << 20) | (c >> 2), pi, t, DOM_FIX], key)
            prod = rnd[c % 4] * n_s
            c += 1
            if (prod & 0xffffffff) < thr:           # Lemire rejection
                continue
            i = mem[prod >> 32]
            if d > 0 and valid[i] and not marks[i]:
                marks[i] = 1
                d -= 1
            elif d < 0 and marks[i]:
                marks[i] = 0
                d += 1
        for i in mem:
            out[i] = int(bool(valid[i]) and (marks[i] ^ int(flip)))
    return out
