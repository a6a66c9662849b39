"""scoary_score_spa (spec S25) on the GPU against the plain-Python restatement (score_spa_spec.py) run on the plan's
rows and S24's outputs as read back from the device: the status exactly, SPA_p's bits = Score_p's at status 0, t^
within 1e-9 relative, z within 1e-9 max(1, |z|), SPA_p within 1e-10 relative of the normal tails at the device's own
z (or of the point mass), S24's outputs untouched -- at the shapes of score_spa_cases.py (fewer isolates than lanes, a
word edge, invalid isolates in the middle of a row, q = 1, 3 and 9, one gene and more pairs than wavefronts, a skipped
trait and one at 5 % positives with rare genes of its own; genes of one and two carriers, of all but one, a perfectly
predictive gene of the balanced and of the rare trait, a gene in the span of the covariates) and at three cutoffs: one
that leaves the work list empty, the default, and the least, 0.1, where the list holds every testable pair; a problem
whose pairs fall back, held to the status and to Score_p's bits; then the refusals.  Every instance q = 1 .. 9 runs (n97 .. n199).  Through
score_spa_cases.fabricate, which makes the device list chosen pairs alone: rows of 4099 isolates and of
scoary_score_spa_max_isolates(); the ends of the support on both sides (beyond it, the point mass from either side of
the end, roots next to it); NaN in the rows of every invalid isolate; more pairs than k_spa_select's grid covers in
one stride, a pair's result whatever else is listed, and a scratch buffer left by a longer list."""
import math

import numpy as np
import pytest

import score_spa_cases as sc
import score_spa_spec as sp

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_SIZE = -1, -3
CUTOFFS = {"empty list": 1e3, "default": sp.CUTOFF, "every pair": sp.MIN_CUTOFF}


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
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


_CACHE = {}


def _case(eng, name):
    """The shape's problem on the device, S24's outputs, and the restatement at the least cutoff on what the device
    holds (computed once per shape: a pair at or above a cutoff does not depend on it)."""
    if name not in _CACHE:
        genes, values, cov = sc.fallback_problem() if name == "fallback" else sc.problem(name)
        gm = eng.pack_dense(genes)
        plan = eng.score_plan(values, cov, "logistic")
        assert plan.spa_rows is None                                  # nothing of S25 is uploaded before its first call
        score = eng.score(gm, plan)
        before = {k: v.clone() for k, v in score.items()}
        eng.score_spa(gm, plan, score, sp.MIN_CUTOFF)
        host = {k: v.cpu().numpy() for k, v in score.items()}
        every = sc.restate(plan.spa_rows.cpu().numpy(), plan.rows.cpu().numpy()[:, 1], plan.valid_host,
                           plan.chol.cpu().numpy(), genes, host, sp.MIN_CUTOFF)
        _CACHE[name] = (genes, gm, plan, score, before, host, every)
    return _CACHE[name]


def _hold(res, host, w, t, g, where):
    """The device's outputs ``res`` of the pair (t, g) against the restatement's ``w``: the status exactly; at status
    0 and 2 Score_p's bits (and zeros at 0); at status 1 t^ within 1e-9 relative, z within 1e-9 max(1, |z|), infinite
    t^ and z = 0 on a side beyond the support or at the point mass, p within 1e-10 relative of the normal tails at
    the device's own z (the restatement's tail on such a side)."""
    assert int(res["status"][t, g]) == w["status"], where + (float(host["stat"][t, g]),)
    if w["status"] != 1:
        assert _bits(res["p"][t, g]) == _bits(host["p"][t, g]), where
        if w["status"] == 0:
            assert not res["z"][t, g].any() and not res["t"][t, g].any(), where
        return
    tails = []
    for s in range(2):
        t_dev, z_dev = float(res["t"][t, g, s]), float(res["z"][t, g, s])
        if math.isinf(w["t"][s]):                                      # the point mass, or beyond the support
            assert t_dev == w["t"][s] and z_dev == 0.0, where + (s, t_dev, z_dev)
            tails.append(w["tails"][s])
            continue
        assert abs(t_dev - w["t"][s]) <= 1e-9 * abs(w["t"][s]), where + (s, t_dev, w["t"][s])
        assert abs(z_dev - w["z"][s]) <= 1e-9 * max(1.0, abs(w["z"][s])), where + (s, z_dev, w["z"][s])
        tails.append(sc.normal_tail(z_dev))
    ref = min(1.0, tails[0] + tails[1])
    assert abs(float(res["p"][t, g]) - ref) <= 1e-10 * ref, where + (float(res["p"][t, g]), ref)


@pytest.mark.parametrize("cutoff", list(CUTOFFS))
@pytest.mark.parametrize("name", list(sc.EVERY_PAIR))
def test_score_spa_matches_the_restatement(eng, name, cutoff):
    import torch
    N, G, c = sc.SHAPES[name]
    genes, gm, plan, score, before, host, every = _case(eng, name)
    assert plan.skipped == [None, "one_class", None] and plan.q == c + 1
    res = {k: v.cpu().numpy() for k, v in eng.score_spa(gm, plan, score, CUTOFFS[cutoff]).items()}
    torch.cuda.synchronize()
    for k in score:                                                    # S24's outputs are read, never written
        assert torch.equal(score[k], before[k]), k
    assert res["p"].shape == (sc.T, G) and res["z"].shape == res["t"].shape == (sc.T, G, 2)
    assert res["status"].dtype == np.int32
    want = sc.at_cutoff(every, host, CUTOFFS[cutoff])
    counts, rare = [0, 0, 0], 0
    for t in range(sc.T):
        for g in range(G):
            w, where = want[t][g], (name, cutoff, t, g)
            assert w["status"] != 2, where                             # score_spa_cases.py: no problem has one
            _hold(res, host, w, t, g, where)
            counts[w["status"]] += 1
            rare += t == 2 and w["status"] == 1
    if cutoff == "empty list":
        assert counts[1] == 0
    else:
        assert counts[1] >= (3 if G >= 70 else 1) and counts[0] >= G   # the skipped trait (and the pairs below)
        if G >= 70:                                                    # the rare trait's own pairs (5 % at n130, n600)
            assert rare >= 5 and res["status"][2, 3] == 1
            if c <= 2:                                                 # its own perfectly predictive gene: a point mass
                assert res["t"][2, 3, 0] == math.inf                   # (eight covariates move it off the end)
            if name in ("n113", "n150"):                               # three and five leave it there, four, six and
                assert res["t"][2, 3, 0] == math.inf                   # seven do not
            elif c > 2:
                assert math.isfinite(res["t"][2, 3, 0])
            if sc.RARE[N] < 0.1:                                       # the regime S25 is for: Score_p far too small
                assert max(res["p"][2, g] / host["p"][2, g] for g in range(3)) > 1e3
    if cutoff == "every pair":
        assert counts[1] == int((host["stat"] >= sp.MIN_CUTOFF ** 2).sum())
        if name == "n64":                                              # more work items than wavefronts launched
            assert counts[1] > 4 * ((sc.T * G + 15) // 16)
    if G >= 70 and cutoff != "empty list":
        assert res["t"][0, G - 4, 0] == math.inf and res["status"][0, G - 4] == 1   # the perfectly predictive gene
        assert res["status"][0, G - 5] == 0 and res["p"][0, G - 5] == 1.0            # in the span of the covariates


def test_pairs_that_fall_back_keep_score_p(eng):
    """score_spa_cases.fallback_problem at the least cutoff: the two pairs of the rare trait whose lower z has the
    wrong sign are status 2 on the device too, with Score_p's bits; every other pair has the restatement's status and,
    at status 0, Score_p's bits (the values at status 1 are held in n130 itself, which differs in three cells)."""
    genes, gm, plan, score, _before, host, every = _case(eng, "fallback")
    res = {k: v.cpu().numpy() for k, v in eng.score_spa(gm, plan, score, sp.MIN_CUTOFF).items()}
    want = np.array([[r["status"] for r in row] for row in every])
    assert np.array_equal(res["status"], want)
    G = len(genes)
    assert (want == 2).sum() == 2 and want[2, G - 1] == 2 and want[2, G - 2] == 2
    for t in range(sc.T):
        for g in range(G):
            if want[t, g] != 1:
                assert _bits(res["p"][t, g]) == _bits(host["p"][t, g]), (t, g)
    assert (res["p"][want == 2] > 0.5).all()                           # statistics of 0.08: nothing lost


def _listed(eng, gm, plan, genes, score, pairs, U=None, cutoff=sp.MIN_CUTOFF):
    """score_spa with S24's outputs ``score`` (numpy) fabricated so that the device lists exactly ``pairs`` (U moved
    where ``U`` says): (the device's outputs as numpy, the fabricated outputs, the restatement of ``pairs`` as a
    dict), the pairs held to the restatement and every other pair to status 0, Score_p's bits and zeros."""
    import torch
    fab = sc.fabricate(score, pairs, U)
    dev = {k: torch.from_numpy(fab[k]).to(eng.device) for k in ("U", "b", "Vg", "stat", "p")}
    res = {k: v.cpu().numpy() for k, v in eng.score_spa(gm, plan, dev, cutoff).items()}
    want = sc.restate(plan.spa_rows.cpu().numpy(), plan.rows.cpu().numpy()[:, 1], plan.valid_host,
                      plan.chol.cpu().numpy(), genes, fab, cutoff, pairs=pairs)
    for t, g in pairs:
        _hold(res, fab, want[t, g], t, g, (t, g))
    _unlisted(res, fab, pairs)
    return res, fab, want


def _unlisted(res, score, pairs):
    """Every pair outside ``pairs``: status 0, the bits of Score_p, zeros."""
    rest = np.ones(res["status"].shape, dtype=bool)
    rest[tuple(np.array(pairs).T)] = False
    assert not res["status"][rest].any() and not res["z"][rest].any() and not res["t"][rest].any()
    assert np.array_equal(_bits(res["p"])[rest], _bits(score["p"])[rest])
    assert np.all(res["status"][~rest] != 0)


def _s24(eng, genes, values, cov):
    gm = eng.pack_dense(genes)
    plan = eng.score_plan(values, cov, "logistic")
    score = eng.score(gm, plan)
    return gm, plan, score, {k: v.cpu().numpy() for k, v in score.items()}


@pytest.mark.parametrize("name", list(sc.SUBSET))
def test_long_rows(eng, name):
    """65 strides of the lanes with a short last one (N = 4099: a word tail, and a tail of the tiled matrix's groups of
    four words), and scoary_score_spa_max_isolates() itself, 1024 isolates a lane: the listed pairs of
    score_spa_cases.LISTED, the only ones restated, at the default cutoff."""
    N, G, c = sc.SHAPES[name]
    if name == "n65536":
        assert N == eng.score_spa_max_isolates()
    genes, values, cov = sc.problem(name)
    gm, plan, _score, host = _s24(eng, genes, values, cov)
    assert plan.skipped == [None, "one_class", None] and plan.q == c + 1 and plan.N == N
    pairs = list(sc.LISTED[name])
    res, _fab, want = _listed(eng, gm, plan, genes, host, pairs, cutoff=sp.CUTOFF)
    assert all(want[pair]["status"] == 1 for pair in pairs)
    if name == "n4099":
        assert len(pairs) == 12 and res["t"][0, G - 4].tolist() == [math.inf, -math.inf] and res["t"][2, 3, 0] == math.inf
        assert all(res["p"][2, g] > 1e3 * host["p"][2, g] for g in range(3))
        assert sum(math.isfinite(x) and x != 0.0 for x in res["t"].ravel().tolist()) == 21


def test_the_ends_of_the_support_on_both_sides(eng):
    """score_spa_cases.ends_problem: the perfectly anti-predictive gene (U < 0: the point mass of side 1, nothing on
    side 0) as it is; then U moved by fabricate to s_end (1 + k 1e-9) -- k = 3 beyond the support, k = +-0.5 the point
    mass -- and to s_end (1 - delta), delta = 1e-2 and 1e-4, a root next to the end, with s_end = s_hi (side 0) and
    |s_lo| (side 1).  0.5e-9 and 3e-9 are far from the 1e-16 by which the device's ends differ from fsum's."""
    genes, values, cov = sc.ends_problem()
    G = len(genes)
    gm, plan, score, host = _s24(eng, genes, values, cov)
    real = {k: v.cpu().numpy() for k, v in eng.score_spa(gm, plan, score, sp.MIN_CUTOFF).items()}
    P = (plan.spa_rows.cpu().numpy(), plan.rows.cpu().numpy()[:, 1], plan.valid_host, plan.chol.cpu().numpy(), genes)
    anti = sc.restate(*P, host, sp.MIN_CUTOFF, pairs=[(0, G - 1), (0, G - 5)])
    for g in (G - 1, G - 5):
        _hold(real, host, anti[0, g], 0, g, ("as it is", g))
    w = anti[0, G - 1]
    assert host["U"][0, G - 1] < 0.0 and w["status"] == 1 and w["t"] == [math.inf, -math.inf]
    assert real["t"][0, G - 1].tolist() == [math.inf, -math.inf] and not real["z"][0, G - 1].any()
    mass = sp.point_mass(sc.items_of(*P, host, 0, G - 1), False)
    assert w["tails"][0] == 0.0 and mass > 0.0 and abs(real["p"][0, G - 1] - mass) <= 1e-10 * mass
    assert real["t"][0, G - 5].tolist() == [math.inf, -math.inf]          # trait 0 itself: the same mass, on side 0
    assert abs(real["p"][0, G - 5] - real["p"][0, G - 1]) <= 1e-9 * mass

    U, what = sc.ends_moves(*P, host)
    pairs = list(U)
    res, _fab, want = _listed(eng, gm, plan, genes, host, pairs, U)
    seen = {}
    for pair, (side, kind, v) in what.items():
        assert want[pair]["status"] == 1 and res["status"][pair] == 1, (pair, side, kind, v)
        seen[side, kind, v] = seen.get((side, kind, v), 0) + 1
        far = -math.inf if side else math.inf
        if kind == "k":
            assert res["t"][pair][side] == far and res["z"][pair][side] == 0.0 and want[pair]["t"][side] == far
            assert (want[pair]["tails"][side] == 0.0) == (v > 1.0)
        else:
            assert math.isfinite(res["t"][pair][side]) and abs(res["t"][pair][side]) > 10.0
    assert all(seen[side, "k", k] == 1 for side in (0, 1) for k in sc.ENDS_K)
    assert all(seen[side, "delta", d] >= 2 for side in (0, 1) for d in sc.ENDS_DELTA)


@pytest.mark.parametrize("name", ["n65", "n150"])
def test_invalid_isolates_are_skipped_by_their_bit(eng, name):
    """S25: isolates outside the valid set and pad bits are skipped by the validity bit, never by relying on zero
    rows.  NaN at every invalid isolate of every row of spa_rows and of S24's rows, every bit of the tiled matrix at
    and past isolate N set: the outputs keep their bits (q = 9 and q = 6)."""
    import torch
    from types import SimpleNamespace
    from scoary_amd.engine import GeneMatrix
    N, G, c = sc.SHAPES[name]
    genes, gm, plan, score, _before, _host, _every = _case(eng, name)
    good = {k: v.cpu().numpy() for k, v in eng.score_spa(gm, plan, score, sp.MIN_CUTOFF).items()}
    T, q = sc.T, c + 1
    invalid = torch.from_numpy(~plan.valid_host).to(eng.device)                       # [T, N]
    assert int(invalid.sum()) >= N + 2 * 3                                            # a whole trait and more
    poisoned = SimpleNamespace(valid=plan.valid, chol=plan.chol)
    for key in ("spa_rows", "rows"):
        rows = getattr(plan, key).clone()
        rows.masked_fill_(invalid[:, None, :], float("nan"))
        assert int(torch.isnan(rows).sum()) == (q + 1) * int(invalid.sum())
        setattr(poisoned, key, rows)
    tiled = gm.tiled.clone()
    for w in range(N // 32, tiled.shape[0] * 4):
        fill = -1 if 32 * w >= N else -(1 << (N - 32 * w))           # as int32: the bits from N - 32 w up
        tiled[w // 4, :, w % 4] |= fill
    outs = [torch.full((T * G * k,), float("nan"), dtype=torch.float64, device=eng.device) for k in (1, 2, 2)]
    outs.append(torch.full((T * G,), 77, dtype=torch.int32, device=eng.device))
    scratch = torch.zeros(int(eng.lib.scoary_score_spa_scratch_bytes(G, T)), dtype=torch.uint8, device=eng.device)
    assert _raw(eng, GeneMatrix(tiled, G, N), poisoned, score, G, T, N, q, sp.MIN_CUTOFF ** 2, outs, scratch) == 0
    torch.cuda.synchronize()
    assert (good["status"] == 1).sum() >= 100
    for o, key in zip(outs, ("p", "z", "t", "status")):
        got = o.cpu().numpy()
        if key == "status":
            assert np.array_equal(got, good[key].ravel())
        else:
            assert not np.isnan(got).any(), key
            assert np.array_equal(_bits(got), _bits(good[key].ravel())), key


def test_select_strides_and_the_list_is_free(eng):
    """score_spa_cases.wide_problem, 525 000 pairs: k_spa_select's 2048 blocks of 256 lanes take a second stride.
    64 listed pairs (pair 0, the last, both sides of pair 524 288, ten neighbours) are held to the restatement and
    every other pair to Score_p's bits.  Listed next to 20 000 others they keep their bits: sums is indexed by list
    position and the list's order comes from atomics, but a pair's result does not depend on the list.  Then the
    first list again on the scratch buffer the longer list left: the first run's outputs bit for bit."""
    import torch
    N, G, T = sc.WIDE
    genes, values, cov = sc.wide_problem()
    gm, plan, _score, host = _s24(eng, genes, values, cov)
    assert T * G > 2048 * 256 and plan.skipped == [None] * T and plan.q == 1
    pairs = sc.wide_listed(host["stat"])
    assert len(pairs) == 64
    first, fab1, want = _listed(eng, gm, plan, genes, host, pairs)
    assert all(w["status"] == 1 for w in want.values())

    rng = np.random.default_rng(sc.WIDE_SEED + 2)
    free = host["stat"] >= sp.MIN_CUTOFF ** 2          # pairs a run could list (where U is the rounding residue of 0,
                                                       # a statistic of 1e-31, S25 itself gives z = 1e14 and p = 0)
    free[tuple(np.array(pairs).T)] = False
    others = [divmod(o, G) for o in rng.choice(np.flatnonzero(free.ravel()), 20000, replace=False).tolist()]
    fab2 = sc.fabricate(host, pairs + others)

    def run(fab, scratch):
        dev = {k: torch.from_numpy(fab[k]).to(eng.device) for k in ("U", "b", "Vg", "stat", "p")}
        outs = [torch.full((T * G * k,), float("nan"), dtype=torch.float64, device=eng.device) for k in (1, 2, 2)]
        outs.append(torch.full((T * G,), 77, dtype=torch.int32, device=eng.device))
        assert _raw(eng, gm, plan, dev, G, T, N, 1, sp.MIN_CUTOFF ** 2, outs, scratch) == 0
        torch.cuda.synchronize()
        return {k: o.cpu().numpy().reshape(first[k].shape) for k, o in zip(("p", "z", "t", "status"), outs)}

    scratch = torch.zeros(int(eng.lib.scoary_score_spa_scratch_bytes(G, T)), dtype=torch.uint8, device=eng.device)
    second = run(fab2, scratch)
    at = tuple(np.array(pairs).T)
    for k in ("p", "z", "t"):
        assert np.array_equal(_bits(second[k][at]), _bits(first[k][at])), k
    assert np.array_equal(second["status"][at], first["status"][at])
    there = tuple(np.array(others).T)
    assert np.isin(second["status"][there], (1, 2)).all() and (second["status"][there] == 1).sum() >= 19000
    assert ((second["p"][there] > 0.0) & (second["p"][there] <= 1.0)).all()
    _unlisted(second, fab2, pairs + others)
    assert int(scratch[:4].view(torch.int32)[0]) == 20064             # the longer list's counter, list and sums
    third = run(fab1, scratch)
    for k in ("p", "z", "t"):
        assert np.array_equal(_bits(third[k]), _bits(first[k])), k
    assert np.array_equal(third["status"], first["status"])


def _raw(eng, gm, plan, score, G, T, N, q, cutoff2, outs, scratch, missing=()):
    ptr = eng._ptr
    ins = [gm.tiled, plan.spa_rows, plan.rows, plan.valid, plan.chol] + [score[k] for k in ("U", "b", "Vg", "stat", "p")]
    a = [None if k in missing else ptr(x) for k, x in enumerate(ins)]
    o = [None if 10 + k in missing else ptr(x) for k, x in enumerate(list(outs) + [scratch])]
    return eng.lib.scoary_score_spa(eng.h, *a, G, T, N, q, cutoff2, *o, eng._stream())


def test_stale_outputs_and_refusals(eng):
    """Outputs that start as garbage are written for every pair and untouched behind; a refusal is a status code with
    a message, launches nothing and leaves the outputs as they were."""
    import torch
    name = "n65"
    N, G, c = sc.SHAPES[name]
    genes, gm, plan, score, _before, host, _every = _case(eng, name)
    T, q, tail = sc.T, c + 1, 32
    good = {k: v.cpu().numpy() for k, v in eng.score_spa(gm, plan, score, sp.MIN_CUTOFF).items()}

    def garbage():
        return [torch.full((T * G * k + tail,), float("nan"), dtype=torch.float64, device=eng.device)
                for k in (1, 2, 2)] + [torch.full((T * G + tail,), 77, dtype=torch.int32, device=eng.device)]

    nbytes = int(eng.lib.scoary_score_spa_scratch_bytes(G, T))
    assert nbytes >= 256 + 4 * T * G and eng.lib.scoary_score_spa_scratch_bytes(0, T) == 0
    assert eng.score_spa_max_isolates() >= 16320
    scratch = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=eng.device)
    outs = garbage()
    assert _raw(eng, gm, plan, score, G, T, N, q, sp.MIN_CUTOFF ** 2, outs, scratch) == 0
    torch.cuda.synchronize()
    for o, key in zip(outs, ("p", "z", "t", "status")):
        got = o.cpu().numpy()
        if key == "status":
            assert np.array_equal(got[:-tail], good[key].ravel()) and (got[-tail:] == 77).all()
        else:
            assert np.array_equal(_bits(got[:-tail]), _bits(good[key].ravel())), key
            assert np.isnan(got[-tail:]).all(), key

    outs = garbage()
    c2 = sp.CUTOFF ** 2
    too_many = eng.score_spa_max_isolates() + 1
    for args, code in (((G, T, too_many, q, c2), ERR_SIZE), ((G, T, N, 0, c2), ERR_SIZE), ((G, T, N, 10, c2), ERR_SIZE),
                       ((G, 65536, N, q, c2), ERR_SIZE), ((1 << 30, 4, N, q, c2), ERR_SIZE),
                       ((0, T, N, q, c2), ERR_ARG), ((G, 0, N, q, c2), ERR_ARG), ((G, T, 0, q, c2), ERR_ARG),
                       ((G, T, N, q, 0.0099), ERR_ARG), ((G, T, N, q, float("nan")), ERR_ARG),
                       ((G, T, N, q, float("inf")), ERR_ARG), ((G, T, N, q, -4.0), ERR_ARG)):
        assert _raw(eng, gm, plan, score, *args, outs, scratch) == code, args
        assert b"scoary_score_spa" in eng.lib.scoary_last_error(eng.h)
    assert _raw(eng, gm, plan, score, G, T, too_many, q, c2, outs, scratch) == ERR_SIZE
    assert b"scoary_score_spa_max_isolates" in eng.lib.scoary_last_error(eng.h)
    for missing in range(15):
        assert _raw(eng, gm, plan, score, G, T, N, q, c2, outs, scratch, missing=(missing,)) == ERR_ARG, missing
    assert _raw(eng, gm, plan, score, G, T, N, q, c2, outs, scratch[4:]) == ERR_ARG      # not aligned to 8 bytes
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        got = o.cpu().numpy()
        assert bool((got == 77).all()) if k == 3 else bool(np.isnan(got).all()), k

    for bad in (0.0999, 0.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cutoff"):
            eng.score_spa(gm, plan, score, bad)
    values = np.random.default_rng(1).standard_normal((1, N))
    linear = eng.score_plan(values, None, "linear")
    with pytest.raises(ValueError, match="logistic"):
        eng.score_spa(gm, linear, eng.score(gm, linear))
    with pytest.raises(ValueError, match="score_out"):
        eng.score_spa(gm, plan, {k: v for k, v in score.items() if k != "Vg"})
    with pytest.raises(ValueError, match="score_out"):
        eng.score_spa(gm, plan, dict(score, U=score["U"][:, :-1]))
    other = _case(eng, "n64")
    with pytest.raises(ValueError, match="the plan has 65 isolates, the gene matrix 64"):
        eng.score_spa(other[1], plan, score)
    handmade = eng.score_plan_of({k: getattr(plan, k + "_host") for k in ("rows", "valid", "chol", "rss")} |
                                 dict(n=plan.n, coef=plan.coef, skipped=plan.skipped), "logistic")
    with pytest.raises(ValueError, match="no fitted values"):
        eng.score_spa(gm, handmade, score)
