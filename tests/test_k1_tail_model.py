"""K1's claimed tail on the CPU: the library's own split (k1_tail_split of
k_consts.h, through tests/k1_tail_model.py) at every boundary of the item
count, for grids of 1, 8, 256 and 304 CUs.

Per size class the counts are, with W = 16 x CUs waves and thr the threshold in
steps per wave (the split's floor and the library's default):
  2 W c (-1, +0, +1), c = thr-1, thr, thr+1   the last launch without a tail and
                                              the first ones with it
  2 (8 W + k), k = 1, 5, 9, 61 (and one       cg = 9, cg_s = 8: pools of 1..16
  item less)                                  chunks (fewer than sub-pools), a cut
                                              last chunk, an odd last item
  1 Mi, 1 Mi + 1                              the headline and its odd neighbour
"""
import random

import pytest

from . import k1_rounds_model as m
from . import k1_tail_model as t

CUS = (1, 8, 256, 304)


def _counts(cus):
    c = t.consts()
    W = 16 * cus
    out = set()
    for thr in (c["floor"], c["default_min"]):
        for steps in (thr - 1, thr, thr + 1):
            out.update(2 * W * steps + d for d in (-1, 0, 1))
    for k in (1, 5, 9, 61):
        out.update((2 * (8 * W + k), 2 * (8 * W + k) - 1))
    out.update((1 << 20, (1 << 20) + 1))
    return sorted(out)


@pytest.fixture(scope="module")
def plans():
    """{(cus, n): (W, ngroups, cg, (cg_s, pool0, nchunks, per))} for every count whose cg reaches the floor."""
    keys = [(cus, n) for cus in CUS for n in _counts(cus) if t.tail_on(n, cus, t.consts()["floor"])]
    geo = [t.geometry(n, cus) for cus, n in keys]
    splits = t.library_splits([(ng, W) for W, ng, _ in geo])
    return {k: g + (s,) for k, g, s in zip(keys, geo, splits)}


def test_constants():
    c = t.consts()
    assert c["pools"] == 16 and c["steps"] in (2, 4) and c["floor"] == 1 << c["shift"]
    assert c["default_min"] >= m.rounds_min_steps() and c["default_min"] >= c["floor"]


def test_the_sweep_holds_the_shapes_it_names(plans):
    c = t.consts()
    few = cut = odd = below = 0
    for (cus, n), (W, ng, cg, (cg_s, pool0, nchunks, per)) in plans.items():
        few += 0 < nchunks < c["pools"]
        cut += (ng - pool0) % c["steps"] != 0
        odd += n % 2
    for cus in CUS:
        below += sum(1 for n in _counts(cus) if not t.tail_on(n, cus, c["floor"]))
    assert few and cut and odd and below


def test_split_tiles_the_batch_once(plans):
    c = t.consts()
    for (cus, n), (W, ng, cg, (cg_s, pool0, nchunks, per)) in plans.items():
        assert cg_s % 4 == 0 and 4 <= cg_s < cg
        assert cg_s == max(4, (cg - (cg >> c["shift"])) // 4 * 4)
        assert pool0 == W * cg_s <= ng
        assert nchunks == -(-(ng - pool0) // c["steps"])
        assert per == [max(0, -(-(nchunks - p) // c["pools"])) for p in range(c["pools"])] and sum(per) == nchunks
        pieces = sorted(t.static_ranges(W, cg_s) + t.chunks(pool0, nchunks, ng))
        assert pieces[0][0] == 0 and pieces[-1][1] == ng, (cus, n)
        assert all(a[1] == b[0] and a[0] < a[1] for a, b in zip(pieces, pieces[1:])), (cus, n)
        # chunk c is chunk c // 16 of sub-pool c % 16
        for p in range(c["pools"]):
            assert len(range(p, nchunks, c["pools"])) == per[p]


def test_static_part_is_k1s_split_of_its_own_items(plans):
    for (cus, n), (W, ng, cg, (cg_s, pool0, nchunks, per)) in plans.items():
        cg2, ranges = m.split(2 * W * cg_s, cus)
        assert cg2 == cg_s and ranges == t.static_ranges(W, cg_s), (cus, n)


def test_below_the_threshold_the_launch_is_todays(plans):
    """The host's decision: under thr steps per wave no counters are passed and
    the kernel's ranges are m.split's (one uniform branch apart)."""
    c = t.consts()
    for cus in CUS:
        W = 16 * cus
        for thr in (c["floor"], c["default_min"]):
            assert not t.tail_on(2 * W * (thr - 1), cus, thr) and not t.tail_on(2 * W * thr - 2 * W, cus, thr)
            assert t.tail_on(2 * W * thr - 2 * W + 1, cus, thr) and t.tail_on(2 * W * thr, cus, thr)
            cg, ranges = m.split(2 * W * (thr - 1), cus)
            assert cg == thr - 1 and len(ranges) == W


def test_every_wave_executes_the_same_barriers(plans):
    S = m.round_steps()
    items = list(plans.items())
    _, rounds = m.library_rounds([v[3][0] for _, v in items])
    for ((cus, n), (W, ng, cg, (cg_s, pool0, nchunks, per))), r in zip(items, rounds):
        walks = {m.walk(g0, g1, W * cg_s, cg_s, S, r)[:2] for g0, g1 in t.static_ranges(W, cg_s)}
        assert all(a + b == r for a, b in walks), (cus, n)  # the static phase alone: k1_rounds(cg_s)
        assert t.wave_barriers(cg_s, S, r) == r + 1, (cus, n)  # the tail path: exactly one more


def _simulate(G, per, rng, fast):
    """G workgroups of 16 waves claim from the sub-pools in a random
    interleaving (waves in `fast` are picked three times as often).  Returns
    (chunks taken, failed claims per wave, heads)."""
    pools = len(per)
    heads = [0] * pools
    live = [(g, p) for g in range(G) for p in range(pools)]
    weights = [3 if w in fast else 1 for w in live]
    taken, failed = [], {w: 0 for w in live}
    while live:
        k = rng.choices(range(len(live)), weights)[0]
        g, p = live[k]
        i = heads[p]
        heads[p] += 1
        if i < per[p]:
            taken.append(pools * i + p)
        else:
            failed[live[k]] += 1
            live.pop(k)
            weights.pop(k)
    return taken, failed, heads


def test_simulated_claims(plans):
    rng = random.Random(7)
    seen = 0
    for (cus, n), (W, ng, cg, (cg_s, pool0, nchunks, per)) in plans.items():
        if cus > 8 or nchunks > 4096:
            continue  # (the same code at sizes a Python loop walks quickly)
        G = W // 16
        waves = [(g, p) for g in range(G) for p in range(16)]
        for fast in (set(), set(rng.sample(waves, len(waves) // 2)), set(waves[:len(waves) // 2])):
            taken, failed, heads = _simulate(G, per, rng, fast)
            assert sorted(taken) == list(range(nchunks)), (cus, n)
            assert set(failed.values()) == {1}
            assert heads == [p + G for p in per]
            seen += 1
    assert seen >= 30
