"""Spec S18's restatement (rank_sd_spec.py) against the consequences the spec states, over 200 random small problems
with ties, missing values and strata of one and two isolates, drawn as test_rank_wy_spec.py draws them; and the fixed
input with a planted driver on which the step-down count is strictly below the single-step one."""
import numpy as np

import rank_sd_spec as sd
import rank_wy_spec as wy
import ranksum_spec as rsp
import vanelteren_spec as vsp

SEED = 0x5EED5EED1818


def _values(rng, N, ties, missing):
    x = np.round(rng.standard_normal(N), 1 if ties else 6)
    if missing:
        x[rng.random(N) < 0.2] = np.nan
    return x


def _genes(rng, G, N):
    genes = (rng.random((G, N)) < rng.uniform(0.1, 0.9, (G, 1))).astype(np.int64)
    if G > 2:
        genes[1] = 0                                    # untestable: m = 0
        genes[2] = 1                                    # untestable: m = n
    if G > 4:
        genes[4] = genes[0]                             # a duplicated gene: a tie group of s_obs
    return genes


def _rows(kind, pr, k, P, base=0):
    if kind == "ranksum":
        return [rsp.perm_row(SEED + k, 0, base + pi, pr["valid"], pr["rc"]) for pi in range(P)]
    return [vsp.perm_row(SEED + k, 0, base + pi, pr["pl"]) for pi in range(P)]


def _problem(rng, k):
    """The k-th random small problem: (kind, genes, the S17 problem, D [G, P], values, strata or None)."""
    N = int(rng.integers(3, 15))
    G = 1 if k % 10 == 0 else int(rng.integers(2, 9))
    P = int(rng.integers(5, 14))
    genes = _genes(rng, G, N)
    vals = _values(rng, N, ties=k % 2 == 0, missing=k % 3 == 0)
    if k % 4 < 2:
        pr = wy.ranksum_problem(genes, vals)
        return "ranksum", genes, pr, wy.permuted(genes, _rows("ranksum", pr, k, P)), vals, None
    S = int(rng.integers(1, 5))
    strata = rng.integers(0, S, N)
    strata[:min(3, N)] = [0, S - 1, S - 1][:min(3, N)]               # strata of size 1 and 2 occur by themselves too
    pv = wy.vanelteren_problem(genes, vals, strata, S)
    return "vanelteren", genes, pv, wy.permuted(genes, _rows("vanelteren", pv, k, P)), vals, (strata, S)


def _solve(kind, genes, vals, strata):
    return wy.ranksum_problem(genes, vals) if kind == "ranksum" else wy.vanelteren_problem(genes, vals, *strata)


def test_the_consequences_the_spec_states():
    rng = np.random.default_rng(1818)
    kinds, sizes, singles, below, above, capped, tied_tops, dup = set(), set(), 0, 0, 0, 0, 0, 0
    for k in range(200):
        kind, genes, pr, D, _vals, _strata = _problem(rng, k)
        G, P = D.shape
        kinds.add(kind)
        if kind == "vanelteren":
            sizes.update(pr["pl"]["n"])
        out = sd.stepdown(D, pr["cc"], pr["iv"], pr["s_obs"])
        mx = wy.maxs(D, pr["cc"], pr["iv"])
        assert np.array_equal(out["u"][0].view(np.uint64), mx.view(np.uint64)), k      # u[0] is S17's maxs
        assert (np.diff(out["u"], axis=0) <= 0).all()
        r, rf, rsd = wy.r_count(D, pr["d"]), wy.r_fwer(mx, pr["s_obs"]), out["r_sd"]
        assert (r <= rsd).all() and (rsd <= rf).all(), (k, r, rsd, rf)
        below += int((rsd < rf).sum())
        above += int((rsd > r).sum())
        top = np.asarray(pr["s_obs"]) == out["ss"][0]                                  # the tie group at rank 0
        assert np.array_equal(rsd[top], rf[top]), k
        tied_tops += int(top.sum() > 1)
        if G == 1:
            singles += 1
            assert np.array_equal(r, rsd) and np.array_equal(rsd, rf), k
        for g in range(G):
            if pr["iv"][g] == 0.0 or abs(pr["d"][g]) <= pr["cc"]:
                capped += 1
                assert pr["s_obs"][g] == 0.0 and rsd[g] == P, (k, g)
        if G > 4:
            dup += 1
            assert rsd[4] == rsd[0], k                                                 # duplicated genes
        # step 3 once more, cell by cell
        for kk in range(G):
            col = [max([0.0] + [wy.stat(D[out["order"][j], pi], pr["cc"], pr["iv"][out["order"][j]])
                                for j in range(kk, G)]) for pi in range(P)]
            assert out["c"][kk] == sum(x >= out["ss"][kk] for x in col), (k, kk)
    assert kinds == {"ranksum", "vanelteren"} and singles == 20 and {1, 2} <= sizes
    assert below > 50 and above > 50 and capped > 100 and dup > 50 and tied_tops > 10


def test_the_order_of_the_genes_does_not_matter():
    """Shuffling the genes of the table leaves every gene's r_sd unchanged, and so does any other order inside the
    tie groups of s_obs."""
    rng = np.random.default_rng(77)
    moved = 0
    for k in range(200):
        kind, genes, pr, D, vals, strata = _problem(rng, k)
        G = len(genes)
        want = sd.stepdown(D, pr["cc"], pr["iv"], pr["s_obs"])
        perm = rng.permutation(G)
        pr2 = _solve(kind, genes[perm], vals, strata)
        assert pr2["s_obs"] == [pr["s_obs"][g] for g in perm]
        got = sd.stepdown(D[perm], pr2["cc"], pr2["iv"], pr2["s_obs"])
        assert np.array_equal(got["r_sd"], want["r_sd"][perm]), k
        moved += int(not np.array_equal(got["order"], want["order"]))
        # inside the tie groups: ties by DEscending gene index instead
        s_obs = np.asarray(pr["s_obs"])
        other = np.asarray(sorted(range(G), key=lambda g: (-s_obs[g], -g)), dtype=np.int64)
        alt = sd.stepdown(D, pr["cc"], pr["iv"], pr["s_obs"], order=other)
        assert np.array_equal(alt["r_sd"], want["r_sd"]), k
    assert moved > 100


def test_two_batches_are_one():
    """c adds over permutation batches (a column belongs to one batch); r_sd does not: the tail runs once."""
    rng = np.random.default_rng(5)
    for k in range(200):
        _kind, _genes_, pr, D, _vals, _strata = _problem(rng, k)
        P = D.shape[1]
        cut = P // 2
        whole = sd.stepdown(D, pr["cc"], pr["iv"], pr["s_obs"])
        a = sd.stepdown(D[:, :cut], pr["cc"], pr["iv"], pr["s_obs"])
        b = sd.stepdown(D[:, cut:], pr["cc"], pr["iv"], pr["s_obs"])
        assert np.array_equal(whole["c"], a["c"] + b["c"]), k
        assert np.array_equal(whole["r_sd"], sd.tail(a["c"] + b["c"], whole["ss"], whole["order"])), k
        assert np.array_equal(whole["u"][0], np.concatenate([a["u"][0], b["u"][0]]))


def test_a_planted_driver_separates_step_down_from_single_step():
    """One driver among null genes: the noise genes are compared with the maximum over the noise alone, so their
    step-down counts are below the single-step ones -- strictly, for at least one gene."""
    _genes_, _values_, pr, _D, out, r, rf = sd.planted_problem()
    rsd = out["r_sd"]
    assert out["order"][0] == 0 and out["order"][1] == 1                 # the driver, then its weaker copy
    assert (r <= rsd).all() and (rsd <= rf).all()
    assert rsd[0] == rf[0] and (rsd < rf).any()
    assert (sd.adjusted_p(rsd, 99) <= sd.adjusted_p(rf, 99)).all() and sd.adjusted_p(rsd, 99).max() <= 1.0
