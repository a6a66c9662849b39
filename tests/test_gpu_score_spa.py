"""scoary_score_spa (spec S25) on the GPU against the plain-Python restatement (score_spa_spec.py) run on the plan's
rows and S24's outputs as read back from the device: the status exactly, SPA_p's bits = Score_p's at status 0, t^
within 1e-9 relative, z within 1e-9 max(1, |z|), SPA_p within 1e-10 relative of the normal tails at the device's own
z (or of the point mass), S24's outputs untouched -- at the shapes of score_spa_cases.py (fewer isolates than lanes, a
word edge, invalid isolates in the middle of a row, q = 1, 3 and 9, one gene and more pairs than wavefronts, a skipped
trait and one at 5 % positives with rare genes of its own; genes of one and two carriers, of all but one, a perfectly
predictive gene of the balanced and of the rare trait, a gene in the span of the covariates) and at three cutoffs: one
that leaves the work list empty, the default, and the least, 0.1, where the list holds every testable pair; a problem
whose pairs fall back, held to the status and to Score_p's bits; then the refusals."""
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


@pytest.mark.parametrize("cutoff", list(CUTOFFS))
@pytest.mark.parametrize("name", list(sc.SHAPES))
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
            assert int(res["status"][t, g]) == w["status"], where + (float(host["stat"][t, g]),)
            counts[w["status"]] += 1
            rare += t == 2 and w["status"] == 1
            if w["status"] == 0:
                assert _bits(res["p"][t, g]) == _bits(host["p"][t, g]), where
                assert not res["z"][t, g].any() and not res["t"][t, g].any(), where
                continue
            tails = []
            for s in range(2):
                t_dev, z_dev = float(res["t"][t, g, s]), float(res["z"][t, g, s])
                if math.isinf(w["t"][s]):                              # the point mass, or beyond the support
                    assert t_dev == w["t"][s] and z_dev == 0.0, where + (s, t_dev, z_dev)
                    tails.append(w["tails"][s])
                    continue
                assert abs(t_dev - w["t"][s]) <= 1e-9 * abs(w["t"][s]), where + (s, t_dev, w["t"][s])
                assert abs(z_dev - w["z"][s]) <= 1e-9 * max(1.0, abs(w["z"][s])), where + (s, z_dev, w["z"][s])
                tails.append(sc.normal_tail(z_dev))
            ref = min(1.0, tails[0] + tails[1])
            assert abs(float(res["p"][t, g]) - ref) <= 1e-10 * ref, where + (float(res["p"][t, g]), ref)
    if cutoff == "empty list":
        assert counts[1] == 0
    else:
        assert counts[1] >= (3 if G >= 70 else 1) and counts[0] >= G   # the skipped trait (and the pairs below)
        if G >= 70:                                                    # the rare trait's own pairs (5 % at n130, n600)
            assert rare >= 5 and res["status"][2, 3] == 1
            if c <= 2:                                                 # its own perfectly predictive gene: a point mass
                assert res["t"][2, 3, 0] == math.inf                   # (eight covariates move it off the end)
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
