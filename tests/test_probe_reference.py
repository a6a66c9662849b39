"""The numpy reference of the permutation probes (tests/probe_regions.py) against the CPU oracle, no GPU:
labels -> minority rows -> float64 matrix product -> interval compare must give orc_permute_r's own r on
every gene when the intervals are the oracle's acceptance rule, converted gene order -> slot order the way
k_lists_crit does it.  This pins the helper, the flip rule and both region conversions before any kernel
is involved."""
import numpy as np
import pytest

import probe_regions as pr


@pytest.mark.parametrize("G,N,P,seed", [(45, 65, 200, 3), (60, 333, 130, 4), (50, 1000, 97, 5)])
def test_reference_reproduces_the_oracle_r(G, N, P, seed):
    from oracle import oracle as orc
    traits = pr.probe_traits(N, seed)                       # masked traits, npos = 1 and npos = nval - 1
    genes, names = pr.probe_genes(G, N, traits, seed)
    assert {"absent", "core", "hot0", "cold0", "half+1", "missing1"} <= set(names)
    T = traits.shape[0]
    npos = (traits == 1).sum(1)
    assert npos[3] == 1 and npos[4] == (traits[4] != 2).sum() - 1
    flipped = pr.flip_rule(genes)
    n1 = genes.sum(1, dtype=np.int64)
    if N % 2 == 0:
        assert not flipped[names.index("half")]
    assert flipped[names.index("half+1")] and flipped[names.index("core")] and not flipped[names.index("absent")]
    minority = pr.minority_rows(genes, flipped)
    L = minority.sum(1, dtype=np.int64)
    assert np.array_equal(L, np.minimum(n1, N - n1))
    order = pr.host_order(L)
    pr.check_order(order, L)

    crit = pr.oracle_crit(orc, genes, traits)
    lo, hi1 = pr.slot_regions_from_crit(crit, order, flipped, npos)
    m = pr.slot_limits(L, npos, order)
    pr.check_regions(lo, hi1, m)
    back = pr.gene_order_crit(lo, hi1, order, flipped, npos)       # the two conversions invert each other
    assert np.array_equal(back, crit)

    lab = pr.oracle_labels(orc, 1234 + seed, traits, P)
    assert lab.shape == (T, P, N)
    assert np.array_equal(lab.sum(2), np.broadcast_to(npos[:, None], (T, P)))
    assert not (lab & (traits == 2)[:, None, :]).any()
    u = pr.overlap_counts(minority, lab)
    assert u.max() <= m.max() and np.all(u[:, order, :].max(-1) <= m)
    tb, mb = pr.trait_bits(traits)
    want = orc.permute_r(pr.pack_bits(genes), tb, mb, N, P, 1234 + seed).T
    got = pr.r_ref(u, order, lo, hi1)
    assert np.array_equal(got, want)
    # the same r from the dense form: a = u for a ones-list, npos - u for a zeros-list
    a = np.where(flipped[None, :, None], npos[:, None, None] - u, u)
    base, span = crit[..., 0].astype(np.int64), crit[..., 1].astype(np.int64)
    dense = ((a < base[..., None]) | (a >= (base + span)[..., None])).sum(-1)
    assert np.array_equal(dense, want)
    assert 0 < (want == P).sum() < want.size


def test_region_families_stay_in_their_domain():
    m = np.array([[0, 1, 2, 7, 500], [0, 0, 1, 3, 9]])
    for name, (lo, hi1) in pr.edge_regions(m).items():
        pr.check_regions(lo, hi1, m)
    seen = set()
    for seed in range(200):
        lo, hi1 = pr.random_regions(m, seed)
        seen.add((int(lo[0, 2]), int(hi1[0, 2])))
    assert seen == {(a, b) for a in range(4) for b in range(a, 4)}     # m = 2: all ten pairs are drawn
