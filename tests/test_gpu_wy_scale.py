"""The Westfall-Young kernels (scoary_minp.hip) at the sizes where their launch loops turn over: the p-table fill
over more than one launch of 2^24 entries (A), a table of more than 2^31 bytes under the fill (A) and under the
gathers of k_permute_minp / k_stepdown_minp (C), and --permute-fwer with a rank that has no genes (D).  The chunked
instances over several gene chunks (B) are parameters of test_gpu_minp.py / test_gpu_stepdown.py.  Every test asserts
that its shape reached the path it is there for, so a later change of the launch sizes fails here instead of passing
over nothing."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_minp import ROW_QUADS, _free_port, bits, run_cli
from test_gpu_parity import P_TOL

pytestmark = pytest.mark.gpu

FILL = 1 << 24              # kMinpFillChunk of scoary_minp.hip: table entries per launch of the fill
N = 2000
MARGINS = ((2000, 1000), (1900, 1400))      # (valid isolates, positives) of the two traits of A
PROD_G = 360_000            # genes of the cases past 2^31 bytes: 801 entries per gene on average


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")


@pytest.fixture(scope="module")
def eng():
    from scoary_amd.engine import AssociationEngine
    return AssociationEngine(0)


def support(nval, npos, n):
    n = np.asarray(n, dtype=np.int64)
    return np.maximum(0, npos + n - nval), np.minimum(npos, n)


def synthetic_counts(margins, n, rng):
    """int32 [T, G, 4]: for trait t = (nval, npos) and the gene margins n[t] a table with these margins and an overlap
    count drawn from its support (the tables read the margins only)."""
    out = []
    for (nval, npos), nt in zip(margins, n):
        lo, hi = support(nval, npos, nt)
        a = rng.integers(lo, hi + 1)
        out.append(np.stack([a, npos - a, nt - a, nval - npos - nt + a], axis=1))
    return np.ascontiguousarray(np.stack(out), dtype=np.int32)


@functools.lru_cache(maxsize=None)
def fill_cases():
    """One draw of gene margins over the whole range (0 and nval, the one-entry tables, among them) and three cuts of
    it: "ragged" = its first 24 000 genes; "whole" and "one" = a prefix plus a few genes whose support sizes make the
    total exactly 2 * 2^24 (no ragged launch) and 2^24 + 1 (a last launch of one table)."""
    rng = np.random.default_rng(2400)
    pool = [rng.integers(0, nval + 1, 42_000) for nval, _npos in MARGINS]
    for t, (nval, _npos) in enumerate(MARGINS):
        pool[t][5], pool[t][6] = 0, nval
    size = [hi - lo + 1 for lo, hi in (support(nval, npos, pool[t]) for t, (nval, npos) in enumerate(MARGINS))]
    cum = np.cumsum(size[0] + size[1])
    # a gene margin n <= 1000 (trait 0) / n <= 500 (trait 1) has a support of n + 1 counts
    assert size[0].max() == 1001 and size[1].max() == 501 and cum[-1] > 2 * FILL

    def landed(target):
        k = int(np.searchsorted(cum, target - 2, side="right"))        # the longest prefix that leaves >= 2 entries
        rest = int(target - cum[k - 1])
        extra = []
        while rest > 0:
            take = min(rest, 1502)
            if rest - take == 1:
                take -= 1
            s0 = min(1001, take - 1)
            extra.append((s0 - 1, take - s0 - 1))
            rest -= take
        return tuple(np.concatenate([pool[t][:k], np.array([e[t] for e in extra], dtype=np.int64)]) for t in range(2))
    cases = {"ragged": tuple(p[:24_000] for p in pool), "whole": landed(2 * FILL), "one": landed(FILL + 1)}
    for n in cases.values():
        for a in n:
            a.setflags(write=False)
    return cases


def plan_and_fill(eng, counts, poison=True):
    """scoary_minp_plan + scoary_minp_fill as eng.minp_tables calls them, on outputs and a scratch buffer prefilled
    with NaN bit patterns: the caching allocator hands back the block of the previous build, and an entry that is
    never written would otherwise carry that build's correct value.  -> (off, lo, tab, entries)."""
    import torch
    T, G = int(counts.shape[0]), int(counts.shape[1])
    off = torch.full((T * G + 1,), -1, dtype=torch.int64, device=eng.device)
    lo = torch.full((T, G), -1, dtype=torch.int32, device=eng.device)
    entries = ctypes.c_int64()
    eng._check(eng.lib.scoary_minp_plan(eng.h, eng._ptr(counts), T, G, eng._ptr(off), eng._ptr(lo),
                                        ctypes.byref(entries), eng._stream()), "scoary_minp_plan")
    total = int(entries.value)
    if not poison:
        return off, lo, None, total
    tab = torch.full((total,), float("nan"), dtype=torch.float64, device=eng.device)
    sbytes = int(eng.lib.scoary_minp_fill_scratch_bytes(total))
    assert sbytes == min(total, FILL) * 24                     # a launch's table list and k_fisher's second output
    scratch = torch.full((sbytes // 8,), -1, dtype=torch.int64, device=eng.device)      # all ones: a NaN as a double
    eng._check(eng.lib.scoary_minp_fill(eng.h, eng._ptr(counts), eng._ptr(off), eng._ptr(lo), T, G, total,
                                        eng._ptr(scratch), eng._ptr(tab), eng._stream()), "scoary_minp_fill")
    torch.cuda.synchronize(eng.device)
    return off, lo, tab, total


def enumerated_p(eng, npos, gmar, nval, lo, size, step=3_000_017):
    """eng.fisher's p of every table of the given (trait, gene) rows, row after row, on the device.  The tables are
    enumerated without k_minp_tables -- repeat_interleave of the sizes -- and go through k_fisher in slices of a length
    that does not divide 2^24.  Arguments: int64 device vectors, one element per row."""
    import torch
    dev = eng.device
    row = torch.repeat_interleave(torch.arange(size.numel(), device=dev), size)
    start = torch.cumsum(size, 0) - size
    total = int(row.numel())
    out = torch.empty((total,), dtype=torch.float64, device=dev)
    for s in range(0, total, step):
        r = row[s:s + step]
        x = lo[r] + torch.arange(s, s + r.numel(), device=dev) - start[r]
        tabs = torch.stack([x, npos[r] - x, gmar[r] - x, nval[r] - npos[r] - gmar[r] + x], dim=1).to(torch.int32)
        out[s:s + r.numel()] = eng.fisher(tabs, want_crit=False)[0]
    return out


def same_bits(got, want):
    """Positions at which two float64 device vectors differ in their bits (NaN patterns included)."""
    import torch
    return torch.nonzero(got.view(torch.int64) != want.view(torch.int64)).reshape(-1)


def straddled(off, entries):
    """Rows i whose [off[i], off[i + 1]) holds a multiple of 2^24 strictly inside (off: host int64)."""
    m = np.arange(FILL, entries, FILL, dtype=np.int64)
    i = np.searchsorted(off, m, side="right") - 1
    return np.unique(i[off[i] < m])


# ---- A. the p-table fill across launch boundaries ---------------------------------------------------------------
@pytest.mark.parametrize("case", ["ragged", "whole", "one"])
def test_fill_over_several_launches(eng, case):
    """Synthetic counts of two traits (all 2000 isolates valid with 1000 positives; 1900 valid with 1400 positives,
    whose supports start above 0) over ~19 000 to ~39 000 genes: more than 2^24 entries, so scoary_minp_fill launches
    k_minp_tables and k_fisher a second (and third) time with an entry offset.  off and lo against numpy's integer
    sums, EVERY entry bit for bit against eng.fisher over independently enumerated tables, and ~3000 entries -- the
    two on each side of every multiple of 2^24 and the first and last of both traits among them -- against the oracle
    at the tolerances of test_gpu_parity.py."""
    import torch
    from oracle import oracle as orc
    n = fill_cases()[case]
    T, G = 2, len(n[0])
    rng = np.random.default_rng(2401)
    counts_h = synthetic_counts(MARGINS, n, rng)
    c = counts_h.astype(np.int64).reshape(-1, 4)
    npos, gmar, nval = c[:, 0] + c[:, 1], c[:, 0] + c[:, 2], c.sum(axis=1)
    lo, hi = np.maximum(0, npos + gmar - nval), np.minimum(npos, gmar)
    size = hi - lo + 1
    off = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
    entries = int(off[-1])
    # the shape reaches what it is there for
    if case == "ragged":
        assert entries > FILL + (1 << 20) and entries % FILL > 1
        assert len(straddled(off, entries)) >= 1           # a gene's table lies across two launches
    elif case == "whole":
        assert entries == 2 * FILL
    else:
        assert entries == FILL + 1
    for t, (nv, _np) in enumerate(MARGINS):
        assert (gmar[t * G:(t + 1) * G] == 0).any() and (gmar[t * G:(t + 1) * G] == nv).any()
    assert (size == 1).sum() >= 4 and lo[G:].max() > 0 and lo[:G].max() > 0

    counts = torch.from_numpy(counts_h).to(eng.device)
    off_d, lo_d, tab, total = plan_and_fill(eng, counts)
    assert total == entries
    assert np.array_equal(off_d.cpu().numpy(), off)
    assert np.array_equal(lo_d.cpu().numpy().reshape(-1), lo)

    dev = [torch.from_numpy(np.ascontiguousarray(v)).to(eng.device) for v in (npos, gmar, nval, lo, size)]
    want = enumerated_p(eng, *dev)
    assert want.numel() == entries and not torch.isnan(want).any()
    bad = same_bits(tab, want)
    assert bad.numel() == 0, "%d of %d entries differ, the first at %s" % (bad.numel(), entries, bad[:8].tolist())

    edges = [m + d for m in range(FILL, entries + 1, FILL) for d in (-2, -1, 0, 1)]
    picks = np.concatenate([rng.integers(0, entries, 3000), edges, [0, off[G] - 1, off[G], entries - 1]])
    picks = np.unique(picks[picks < entries]).astype(np.int64)
    assert {FILL - 1, FILL} <= set(picks.tolist())
    i = np.searchsorted(off, picks, side="right") - 1
    x = lo[i] + picks - off[i]
    tabs = np.stack([x, npos[i] - x, gmar[i] - x, nval[i] - npos[i] - gmar[i] + x], axis=1).astype(np.int32)
    assert tabs.min() >= 0
    _odds, o_p = orc.fisher_many(tabs)
    got = tab[torch.from_numpy(picks).to(eng.device)].cpu().numpy()
    big = o_p > 1e-280
    print("%s: G = %d, %d entries, %d launches; %d oracle entries: max |dp| %.3g, max relative %.3g over %d"
          % (case, G, entries, -(-entries // FILL), len(picks), np.max(np.abs(got - o_p)),
             np.max(np.abs(got[big] - o_p[big]) / o_p[big]), big.sum()))
    assert np.max(np.abs(got - o_p)) < P_TOL
    assert big.sum() > 1000 and np.max(np.abs(got[big] - o_p[big]) / o_p[big]) < 1e-11


def test_fill_of_a_table_past_2_pow_31_bytes(eng):
    """One trait of 1000 positives among 2000 isolates, 360 000 genes with margins 600 ... 1000 (601 to 1001 entries
    each): the headline size of a trait group -- eighteen launches of the fill, entry offsets whose byte offsets pass
    2^31.  off against torch's int64 cumsum, the table bit for bit against eng.fisher over all tables of 4096 random
    genes, of every gene that lies across a multiple of 2^24 and of the first and last gene."""
    import torch
    G = PROD_G
    rng = np.random.default_rng(3100)
    counts_h = synthetic_counts(((2000, 1000),), [rng.integers(600, 1001, G)], rng)
    counts = torch.from_numpy(counts_h).to(eng.device)
    off_d, lo_d, tab, entries = plan_and_fill(eng, counts)
    assert entries * 8 > (1 << 31) + (1 << 27)
    c = counts[0].to(torch.int64)
    npos, gmar, nval = c[:, 0] + c[:, 1], c[:, 0] + c[:, 2], c.sum(dim=1)
    lo = torch.clamp(npos + gmar - nval, min=0)
    size = torch.minimum(npos, gmar) - lo + 1
    assert int(off_d[0]) == 0 and torch.equal(off_d[1:], torch.cumsum(size, 0)) and int(off_d[-1]) == entries
    assert torch.equal(lo_d.reshape(-1).to(torch.int64), lo)
    across = straddled(off_d.cpu().numpy(), entries)
    assert len(across) >= 16
    rows = np.unique(np.concatenate([rng.choice(G, 4096, replace=False), across, [0, G - 1]]))
    r = torch.from_numpy(rows).to(eng.device)
    want = enumerated_p(eng, npos[r], gmar[r], nval[r], lo[r], size[r])
    sz = size[r]
    within = torch.arange(want.numel(), device=eng.device) - torch.repeat_interleave(torch.cumsum(sz, 0) - sz, sz)
    where = torch.repeat_interleave(off_d[r], sz) + within
    assert int(where.max()) == entries - 1 and int(where.min()) == 0
    assert not torch.isnan(want).any()
    bad = same_bits(tab[where], want)
    assert bad.numel() == 0, "%d of %d checked entries differ, the first at entry %s" % (
        bad.numel(), want.numel(), where[bad[:8]].tolist())
    print("fill past 2^31 bytes: G = %d, %d entries (%.2f GB), %d launches, %d genes across a launch boundary, "
          "%d entries checked" % (G, entries, entries * 8 / 1e9, -(-entries // FILL), len(across), want.numel()))


# ---- C. both permute kernels over a table of more than 2^31 bytes ------------------------------------------------
def test_permute_kernels_gather_past_2_pow_31_bytes(eng):
    """A's production-size layout from a real matrix (360 000 genes at frequencies 0.3-0.7, 2000 isolates, one trait
    with 1000 positives), the tables filled with random doubles so that a gather from the wrong place shows, 70 random
    label rows (two permutation groups, the last one ragged; rows leave the supports, the clamp is part of the
    contract).  Reference in torch on the device: overlap counts by an fp32 matrix product (0/1 products, sums below
    2^24: exact), one gather, the minimum, and for the step-down a random rank order with p_sorted drawn from the
    successive minima themselves, as test_raw_counts_over_synthetic_tables does."""
    import torch
    from scoary_amd.engine import MinpTables, pack_bits_rows
    G, T, P = PROD_G, 1, 70
    dev = eng.device
    assert eng.quads(N) == ROW_QUADS[N] <= 24                   # the register-resident instances: the headline shape's
    gen = torch.Generator(device=dev)
    gen.manual_seed(7100)
    rng = np.random.default_rng(7100)
    genes = (torch.rand((G, N), device=dev, generator=gen)
             < 0.3 + 0.4 * torch.rand((G, 1), device=dev, generator=gen)).to(torch.uint8)
    gm = eng.pack_dense(genes)
    trait = np.zeros((1, N), dtype=np.uint8)
    trait[0, rng.permutation(N)[:1000]] = 1
    trv = eng.vecrows(pack_bits_rows(trait), N)
    mkv = eng.vecrows(pack_bits_rows(np.ones((1, N), dtype=np.uint8)), N)
    counts, _margins = eng.counts(gm, trv, mkv)
    off, lo, _tab, entries = plan_and_fill(eng, counts, poison=False)
    assert entries * 8 > 1 << 31
    tab = torch.rand((entries,), dtype=torch.float64, device=dev, generator=gen)
    tables = MinpTables(off, lo, tab, entries)
    labels = (rng.random((P, N)) < rng.uniform(0.2, 0.8, (P, 1))).astype(np.uint8)
    perms = eng.vecrows(pack_bits_rows(labels), N)[None].contiguous()

    a = (torch.from_numpy(labels).to(dev).float() @ genes.float().T).to(torch.int64)              # [P, G]
    size = off[1:] - off[:-1]
    rel = a - lo.reshape(1, G).to(torch.int64)
    assert bool((rel < 0).any())                                # the clamp acts
    where = off[:-1][None, :] + torch.minimum(torch.clamp(rel, min=0), (size - 1)[None, :])
    assert int(where.max()) > 1 << 28                           # entries gathered from beyond 2^31 bytes
    pperm = tab[where]
    want_minp = pperm.amin(dim=1)
    order = torch.randperm(G, device=dev, generator=gen)
    q = torch.flip(torch.cummin(torch.flip(pperm[:, order], dims=(1,)), dim=1).values, dims=(1,))
    pick = torch.randint(0, P, (G,), device=dev, generator=gen)
    ps = torch.sort(q[pick, torch.arange(G, device=dev)]).values
    ps[500:540] = ps[500]                                       # a run of 40 equal values
    assert bool((ps[1:] >= ps[:-1]).all())
    want_c = (q <= ps[None, :]).sum(dim=0)
    # informative: most positions strictly between 0 and P, and the exact-equality case occurs
    assert float(((want_c > 0) & (want_c < P)).double().mean()) > 0.5
    assert int((q == ps[None, :]).sum()) >= 10

    minp = torch.ones((T, P), dtype=torch.float64, device=dev)
    eng.permute_minp(gm, perms, tables, minp)
    assert np.array_equal(bits(minp.cpu().numpy().reshape(-1)), bits(want_minp.cpu().numpy()))
    c = torch.zeros((T, G), dtype=torch.int32, device=dev)
    minp_sd = torch.ones((T, P), dtype=torch.float64, device=dev)
    eng.permute_stepdown(gm, perms, tables, order.to(torch.int32).reshape(1, G).contiguous(), ps.reshape(1, G), c,
                         minp=minp_sd)
    assert torch.equal(c.reshape(-1).to(torch.int64), want_c)
    assert np.array_equal(bits(minp_sd.cpu().numpy().reshape(-1)), bits(want_minp.cpu().numpy()))
    print("gathers past 2^31 bytes: G = %d, %d entries (%.2f GB), largest offset gathered %d, %d chunks of the rank "
          "order" % (G, entries, entries * 8 / 1e9, int(where.max()), eng.stepdown_chunks(G, T, P)))


# ---- D. --permute-fwer with a rank that has no genes -------------------------------------------------------------
# seconds: the two-rank sibling (test_cli_permute_fwer_two_ranks_share_the_gpu) takes 5 s on an MI355X box, nearly all
# of it the start of the processes; the margin is for a cold file cache and a busy host
RANKS_TIMEOUT = 60


def test_cli_permute_fwer_with_a_rank_without_genes(tmp_path):
    """Two genes over three ranks (gloo, one GPU): the third rank's shard is empty, and it must still take part in the
    all_reduce(MIN) of the [T, P] minima -- with ones -- before the records are gathered.  The result file is the
    single-process run's, byte for byte; a collective that does not match ends at the time limit instead."""
    from conftest import ROOT
    from scoary_amd.dist import GenePartition
    assert list(GenePartition(2, 3).lengths()) == [1, 1, 0]
    strains = ["iso%02d" % i for i in range(12)]
    rows = {"geneA": [1, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0], "geneB": [1, 0, 1, 0, 1, 1, 0, 1, 0, 0, 1, 0]}
    trait = [1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0]
    gpa, tr = str(tmp_path / "genes.csv"), str(tmp_path / "traits.csv")
    with open(gpa, "w") as f:
        f.write(",".join(["Gene", "Non-unique Gene name", "Annotation", "No. isolates", "No. sequences",
                          "Avg sequences per isolate", "Genome Fragment", "Order within Fragment",
                          "Accessory Fragment", "Accessory Order with Fragment", "QC", "Min group size nuc",
                          "Max group size nuc", "Avg group size nuc"] + strains) + "\n")
        for name, row in rows.items():
            f.write(",".join([name, "", "hypothetical"] + [""] * 11
                             + [("%s_%d" % (name, i) if v else "") for i, v in enumerate(row)]) + "\n")
    with open(tr, "w") as f:
        f.write(",resistance\n" + "".join("%s,%d\n" % (s, v) for s, v in zip(strains, trait)))
    argv = ["-g", gpa, "-t", tr, "--no_pairwise", "-e", "20", "--seed", "1", "-p", "1.0", "--permute-fwer"]
    one = run_cli(argv, tmp_path / "one")
    assert list(one) == ["resistance.results.csv"]
    lines = one["resistance.results.csv"].splitlines()
    assert len(lines) == 3 and "Westfall_Young_p" in lines[0]             # both genes, and the column
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(PYTHONPATH=ROOT + os.pathsep + env.get("PYTHONPATH", ""), SCOARY_SHARE_GPU="1",
               SCOARY_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    three = tmp_path / "three"
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3",
                          "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                          "-m", "scoary_amd"] + argv + ["--no-time", "-o", str(three)],
                         capture_output=True, text=True, timeout=RANKS_TIMEOUT, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    with open(three / "resistance.results.csv", newline="") as f:
        assert f.read() == one["resistance.results.csv"]
