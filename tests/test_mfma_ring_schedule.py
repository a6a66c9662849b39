"""The barrier / LDS-ring schedule of k_permute_mfma, walked on the CPU as the kernel's header states it.

A block streams nh half stages of B through a ring of kRingSlots LDS slots (half n in slot n % kRingSlots); every
wavefront moves kDmaPerHalf LDS-DMA pieces of each half, waits with a counted vmcnt that leaves one half's
pieces outstanding, and executes nh + 1 barriers.  A half is 32 fragments; fragment f is read kBLead fragments
ahead of its MFMAs.  Between barrier n and barrier n + 1 (interval n)

  an early wavefront (0..3)  issues the pieces of half n + 2 right behind the barrier and reads half n;
  a late wavefront (4..7)    reads fragments 16..31 of half n - 1, crosses its half boundary without a barrier,
                             issues the pieces of half n + 2 there, and reads fragments 0..15 of half n (interval
                             0 begins at that boundary).  Its last interval is the tail: fragments 16..31 of
                             half nh - 1 behind barrier nh.  Across the boundary its fragment ring goes on:
                             fragments 0..2 of half n are read in front of the last MFMAs of half n - 1.

At the boundary into a stage (an even half) a wavefront takes the thresholds it fetched one stage earlier and
then fetches the next ones: a late wavefront in front of the pieces it issues there, an early one behind those
of its barrier.  Halves past the end are copies of the last one and go through the same motions.

The model below produces each group's instruction stream from that description and nothing else: it restates the
header, it does not parse the loop, so a change of the loop that the header does not follow is not seen here (the
GPU tests compare r).  Ring depth, issue distance, read lead and pieces per half are computed from the constants
of the sources; the place of the late wavefronts' barrier is taken from the description, and one literal line of
the loop is looked for only to tie this file to the revision it describes -- if that line moves or is rewritten,
re-read the loop against the description above and then bring the pattern up to date.
It is a statement about the schedule, not a simulation of the hardware: vector memory operations retire in issue
order, so behind `s_waitcnt vmcnt(k)` everything but the k youngest has landed, and whatever a wavefront does
behind barrier b happens after everything any wavefront did in front of it.
"""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAGS = 32                     # B fragments of a half stage
MID = FRAGS // 2               # the late wavefronts' barrier: in front of this fragment


@pytest.fixture(scope="module")
def k():
    csrc = os.path.join(ROOT, "scoary_amd", "csrc")
    src = open(os.path.join(csrc, "scoary_mfma.hip")).read()
    common = open(os.path.join(csrc, "scoary_common.hpp")).read()

    def const(text, pat):
        m = re.search(pat, text)
        assert m, pat
        return int(m.group(1))

    c = {}
    for name, pat in (("slots", r"constexpr int kRingSlots = (\d+);"), ("lead", r"constexpr int kBLead = (\d+)"),
                      ("ahead_minus", r"constexpr int kAhead = kRingSlots - (\d+);")):
        m = re.search(pat, src)
        assert m, name
        c[name] = int(m.group(1))
    c["ahead"] = c["slots"] - c["ahead_minus"]
    # kDmaPerHalf = kHalfBytes / kBlockWaves / kFragBytes, kHalfBytes = kStageBytes / 2 = kKSteps * kFragBytes
    assert "constexpr int kStageBytes = 2 * kKSteps * kFragBytes;" in common
    assert "constexpr int kHalfBytes = kStageBytes / 2;" in src
    assert "constexpr int kDmaPerHalf = kHalfBytes / kBlockWaves / kFragBytes;" in src
    ksteps = const(common, r"constexpr int kKSteps = (\d+);")
    waves = const(src, r"constexpr int kBlockWaves = (\d+);")
    assert ksteps % waves == 0
    c["pieces"] = ksteps // waves
    # the counted wait: (kAhead - 1) halves of pieces stay outstanding
    assert 'asm volatile("s_waitcnt vmcnt(%0)" ::"n"((kAhead - 1) * kDmaPerHalf) : "memory");' in src
    # the revision tie (see the module's docstring): the late wavefronts' barrier stands in front of fragment MID
    assert "if (kLate && f == kFrags / 2) barrier();" in src
    return c


def stream(k, nh, late):
    """The instruction stream of one wavefront: ("dma", half, piece) | ("fetch",) | ("take",) | ("wait",) |
    ("barrier", n) | ("read", half, fragment), in program order."""
    ev = []
    for n in range(k["ahead"]):
        ev += [("dma", n, p) for p in range(k["pieces"])]
    nx = [k["ahead"]]

    def issue_half():
        ev.extend(("dma", nx[0], p) for p in range(k["pieces"]))
        nx[0] += 1

    def barrier(n):
        ev.extend([("wait",), ("barrier", n)])

    def boundary(n):           # into half n; the thresholds move at a stage's first half
        if n % 2 == 0:
            if n >= 2:
                ev.append(("take",))
            if n + 2 < nh:
                ev.append(("fetch",))

    def fragments(n, lo, hi, cross):
        for f in range(lo, hi):
            if late and f == MID:
                barrier(n + 1)
            g = f + k["lead"]
            if g < FRAGS:
                ev.append(("read", n, g))
            elif cross:
                ev.append(("read", n + 1, g - FRAGS))
            ev.append(("mfma", n, f))

    if late:
        barrier(0)
        ev += [("read", 0, f) for f in range(k["lead"])]
        for n in range(nh):
            boundary(n)
            issue_half()
            fragments(n, 0, FRAGS, cross=True)
    else:
        for n in range(nh):
            barrier(n)
            issue_half()
            ev += [("read", n, f) for f in range(k["lead"])]
            boundary(n)
            fragments(n, 0, FRAGS, cross=False)
        barrier(nh)
    return ev


def intervals(ev):
    """(event, interval): the index of the last barrier in front of the event, -1 in front of barrier 0."""
    out, cur = [], -1
    for e in ev:
        if e[0] == "barrier":
            assert e[1] == cur + 1, "barriers are executed in order"
            cur = e[1]
        out.append((e, cur))
    return out


NH = range(1, 13)


@pytest.mark.parametrize("nh", NH)
def test_both_groups_execute_the_same_barriers(k, nh):
    for late in (False, True):
        bars = [e[1] for e in stream(k, nh, late) if e[0] == "barrier"]
        assert bars == list(range(nh + 1)), (late, bars)


@pytest.mark.parametrize("nh", NH)
def test_every_fragment_is_read_once_before_its_mfma_and_behind_its_barrier(k, nh):
    for late in (False, True):
        seen = {}
        for pos, (e, iv) in enumerate(intervals(stream(k, nh, late))):
            if e[0] == "read":
                assert iv >= e[1], "late %s: fragment %d of half %d read in interval %d" % (late, e[2], e[1], iv)
                assert (e[1], e[2]) not in seen
                seen[(e[1], e[2])] = pos
            elif e[0] == "mfma":
                assert (e[1], e[2]) in seen, "late %s: MFMA of (%d, %d) without its read" % (late, e[1], e[2])
        assert {h for h, _f in seen} >= set(range(nh))
        for n in range(nh):
            assert sum(1 for h, _f in seen if h == n) == FRAGS


@pytest.mark.parametrize("nh", NH)
def test_barrier_n_makes_half_n_whole(k, nh):
    """The counted wait in front of barrier n leaves at most (kAhead - 1) halves' pieces outstanding, the youngest
    ones; none of them may belong to a half <= n, and an interval's pieces are all issued in front of its wait."""
    left = (k["ahead"] - 1) * k["pieces"]
    for late in (False, True):
        ev = stream(k, nh, late)
        vm, nbar = [], 0
        for i, e in enumerate(ev):
            if e[0] in ("dma", "fetch"):
                vm.append(e)
            elif e[0] == "wait":
                n = ev[i + 1][1]
                assert ev[i + 1][0] == "barrier" and n == nbar
                landed, pending = vm[:len(vm) - left], vm[len(vm) - left:]
                issued = {(x[1], x[2]) for x in landed if x[0] == "dma"}
                for h in range(n + 1):
                    for p in range(k["pieces"]):
                        assert (h, p) in issued, "late %s: piece %d of half %d not landed at barrier %d" % (late, p, h, n)
                # what is issued in interval n - 1 is half n + kAhead - 1, whole, and nothing of a later half
                assert all(x[0] == "fetch" or x[1] <= n + k["ahead"] - 1 for x in vm), (late, n)
                assert {(x[1], x[2]) for x in vm if x[0] == "dma"} >= {
                    (n + k["ahead"] - 1, p) for p in range(k["pieces"])}, (late, n)
                nbar += 1


@pytest.mark.parametrize("nh", NH)
def test_no_slot_receives_a_half_while_the_one_it_holds_may_be_read(k, nh):
    """A piece of half m is issued in some interval b, so after every wavefront has reached barrier b; every read
    of an earlier half of the same slot, by either group, must lie in front of that wavefront's barrier b."""
    streams = [intervals(stream(k, nh, late)) for late in (False, True)]
    reads = [(e[1], iv) for s in streams for e, iv in s if e[0] == "read"]
    for s in streams:
        for e, b in s:
            if e[0] != "dma":
                continue
            for half, iv in reads:
                if half < e[1] and half % k["slots"] == e[1] % k["slots"]:
                    assert iv < b, "half %d issued in interval %d, half %d of its slot read in interval %d" % (
                        e[1], b, half, iv)
    # and the slots read or in flight in one interval are distinct: n - 1, n read, n + 1, n + 2 in flight
    assert k["slots"] >= k["ahead"] + 2


@pytest.mark.parametrize("nh", NH)
def test_thresholds_have_landed_when_they_are_taken(k, nh):
    """fetch ... take: a counted wait between them behind which the fetch is not among the youngest operations;
    and no fetch overwrites thresholds that are still to be taken."""
    left = (k["ahead"] - 1) * k["pieces"]
    for late in (False, True):
        vm, pending, landed = [], None, False
        for e in stream(k, nh, late):
            if e[0] == "dma":
                vm.append(e)
            elif e[0] == "fetch":
                assert pending is None, "late %s: a fetch over thresholds not yet taken" % late
                vm.append(e)
                pending, landed = len(vm) - 1, False
            elif e[0] == "wait" and pending is not None:
                landed = landed or pending < len(vm) - left
            elif e[0] == "take":
                assert pending is not None and landed, "late %s nh %d: thresholds taken before they landed" % (late, nh)
                pending = None
