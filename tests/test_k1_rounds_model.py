"""K1's lockstep rounds, on the CPU: every wave of a launch executes the same
number of workgroup barriers, k1_rounds(cg, S) of k_consts.h, on every path.

A missed barrier would hang a GPU, so the count is checked here before any
kernel runs: tests/k1_rounds_model.py restates K1's range split (grid_for, the
scramble, cg, gend) and walks each wave's path through the 4-step loop (where
it arrives once per S steps), the 2-step and 1-step epilogues and the make-up
loop behind its last store; launches of fewer than kK1RoundsMinSteps steps per
wave have no rounds at all.  k1_rounds and S are the library's own, read
through a host program compiled against k_consts.h."""
import numpy as np
import pytest

from . import k1_rounds_model as m


def _item_counts(cus, S, M):
    W = 16 * m.grid_for(cus, 1 << 40)
    ns = {1, 2, 3, 31, 32, 33, 63, 64, 65, 32 * cus - 1, 32 * cus, 32 * cus + 1}
    for c in (1, 2, 3, 4, 5, 7, S - 1, S, S + 1, S + 3, S + 4, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S + 2, 8 * S,
              M - 1, M, M + 1, M + 2, M + 3, M + S - 1, M + S, M + S + 1, 2 * M + 1):
        ns |= {2 * W * c - 1, 2 * W * c, 2 * W * c + 1, 2 * W * c + 5}
    ns |= {2 * W * (S + 1) - W - 3, 1 << 20, (1 << 20) + 1, 57347, 41160}
    rng = np.random.default_rng(cus)
    ns |= {int(x) for x in rng.integers(1, 2 * W * (M + 3 * S + 1), 12)}
    return sorted(n for n in ns if n >= 1)


@pytest.mark.parametrize("cus", [1, 8, 256, 304])
def test_every_wave_executes_k1_rounds_barriers(cus):
    S, M = m.round_steps(), m.rounds_min_steps()
    assert S >= 4 and S % 4 == 0
    counts = _item_counts(cus, S, M)
    splits = [m.split(n, cus) for n in counts]
    _, want = m.library_rounds([cg for cg, _ in splits])
    seen_loops, seen_short, seen_empty = set(), False, False
    for n, (cg, ranges), rounds in zip(counts, splits, want):
        ngroups = (n + 1) // 2
        assert len(ranges) == 16 * m.grid_for(cus, n)
        # the ranges tile the batch: the barrier changes nothing about who reads what
        busy = sorted(r for r in ranges if r[0] < ngroups)
        assert busy[0][0] == 0 and busy[-1][1] == ngroups
        assert all(a[1] == b[0] for a, b in zip(busy, busy[1:]))
        assert rounds == 0 or cg >= M
        for g0, g1 in ranges:
            in_loop, makeup, passed, loops = m.walk(g0, g1, ngroups, cg, S, rounds)
            what = (n, cus, g0, g1, cg, in_loop, makeup, passed, rounds)
            nsteps = g1 - g0 if g0 < ngroups else 0
            # the round ends a wave passes are those of the steps its 4-step loop runs
            assert passed == nsteps // 4 * 4 // S, what
            if rounds:
                # never more than it owes, so the kernel's `&& owed` never holds a
                # wave back in a launch with rounds: it arrives at every round end
                # it passes, and makes up exactly the ones it did not reach
                assert passed <= rounds and in_loop == passed and makeup == rounds - passed, what
            else:
                assert in_loop == 0 and makeup == 0, what
            # every wave of the launch executes the same number of barriers
            assert in_loop + makeup == rounds, what
            seen_loops.add(tuple(bool(x) for x in loops))
            seen_empty |= g0 >= ngroups
            seen_short |= g0 < ngroups and g1 - g0 < cg and rounds > 0 and makeup > 0
    # the sweep did reach an empty range, a cut one that makes up arrivals, and
    # every mix of the 4/2/1-step loops
    assert seen_empty and seen_short
    assert seen_loops >= {(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)} - {(False,) * 3}


def test_k1_rounds_reads_cg_alone():
    """A full range arrives floor(cg / S) times in its loop and owes nothing
    more; cg below kK1RoundsMinSteps means no barrier at all."""
    S, M = m.round_steps(), m.rounds_min_steps()
    cgs = list(range(0, M + 4 * S + 3)) + [128, 512, 1 << 20]
    _, got = m.library_rounds(cgs)
    assert got == [cg // S if cg >= M else 0 for cg in cgs]
    for cg, rounds in zip(cgs, got):
        in_loop, makeup, passed, _ = m.walk(0, cg, max(cg, 1), cg, S, rounds)
        if cg:
            assert (in_loop, makeup) == (rounds, 0) and passed == cg // S


def test_the_walk_catches_a_wrong_count():
    """The checks above are not true by construction: with one round too few
    a full range passes more round ends than it owes (the kernel's guard would
    have to hold it back), and with one too many it makes up an arrival it
    should have made in its loop."""
    S, M = m.round_steps(), m.rounds_min_steps()
    cg = M + S
    in_loop, makeup, passed, _ = m.walk(0, cg, cg, cg, S, cg // S - 1)
    assert passed > cg // S - 1 and in_loop < passed
    in_loop, makeup, passed, _ = m.walk(0, cg, cg, cg, S, cg // S + 1)
    assert in_loop == passed == cg // S and makeup == 1
