"""K1's order on the CPU (no GPU): the Python restatement of k1_walk / k1_group
(tests/k1_order_model.py) against the library's own arithmetic, read through
the stand-alone, sanitized tests/integration/k1_order_check.cpp.

For the ranges (O0), the window by step (O1) and the window by pass (O2), the
windows dealt scrambled and in launch order:
  - the groups read are a permutation of [0, W cg): with the claimed tail that
    is the static part [0, W cg_s); without it, cut at the batch's end, a cover
    of [0, ngroups) with no group read twice or missed
  - every wave's pass is four groups in the order's stated layout
  - every wave executes k1_rounds(cg) barriers, on the path the kernel's loops
    take (simulate: every statement of the static part, its ring included)
over W = 16 B for B in {1, 8, 255, 256, 304} (65521 cannot divide any of them),
a synthetic B = 65521 with one wave per workgroup, for which both scrambles
are skipped, and every ngroups in a band around W cg for cg in {31, 32, 33, 40,
127, 128}."""
import numpy as np
import pytest

from . import k1_order_model as o
from . import k1_rounds_model as m
from . import k1_tail_model as t

ORDERS = [(o.RANGES, True), (o.WINDOW_STEP, True), (o.WINDOW_STEP, False), (o.WINDOW_PASS, True), (o.WINDOW_PASS, False)]
BS = (1, 8, 255, 256, 304)
CGS = (31, 32, 33, 40, 127, 128)
BAND = 35  # ngroups in [W cg - BAND, W cg + BAND]: cg and cg + 1 steps per wave, windows cut by up to two waves' passes


def test_the_constants_the_model_assumes():
    assert m.rounds_min_steps() == 32 and m.round_steps() == 4
    assert all((16 * b) % o.PRIME and b % o.PRIME for b in BS)


@pytest.fixture(scope="module")
def lib():
    """The check program's line per (order, scramble, B, wv, cg): all cases in a few runs."""
    cases = [(order, scr, b, 16, cg) for order, scr in ORDERS for b in BS for cg0 in CGS for cg in (cg0, cg0 + 1)]
    cases += [(order, scr, o.PRIME, 1, cg) for order, scr in ORDERS for cg in (32, 33)]
    cases = sorted(set(cases))
    return dict(zip(cases, o.library(cases)))


def test_model_equals_library_and_is_a_permutation(lib):
    for (order, scr, b, wv, cg), (run, rounds, csum, perm, layout) in lib.items():
        what = (order, scr, b, wv, cg)
        assert run == o.order_for(order, cg) == (order if cg >= 32 else o.RANGES), what
        assert rounds == (cg // 4 if cg >= 32 else 0), what
        assert perm == 1 and layout == 1, what
        g = o.groups(run, scr, b, wv, cg)
        assert o.checksum(g) == csum, what
        assert np.array_equal(np.sort(g.reshape(-1)), np.arange(b * wv * cg, dtype=np.uint64)), what


def test_walk_equals_groups():
    """The scalar walk the simulation uses names the same groups as the vectorised restatement."""
    for order, scr in ORDERS:
        for b, cg in ((8, 33), (8, 32), (255, 34), (1, 35)):
            g = o.groups(order, scr, b, 16, cg)
            for wg in (0, b // 2, b - 1):
                for tt in (0, 7, 15):
                    first, ss, ps, rfirst, end = o.walk(order, scr, wg, tt, b, 16, cg)
                    want = [first + (s // 4) * ps + (s % 4) * ss if s < cg // 4 * 4 else rfirst + (s % 4) * ss for s in range(cg)]
                    assert list(g[wg, tt]) == want and max(want) < end, (order, scr, b, cg, wg, tt)


def test_window_by_pass_layout():
    """O2 as the issue states it: in pass q wave t reads base + 64 q + 4 t + j, so a wave reads 32 KiB contiguously
    per pass and the workgroup 512 KiB contiguously per round."""
    for scr in (True, False):
        g = o.groups(o.WINDOW_PASS, scr, 256, 16, 128)
        for b in (0, 5, 255):
            base = (o.scramble(b, 256) if scr else b) * 16 * 128
            for q in (0, 1, 31):
                assert [int(x) for x in g[b, :, 4 * q:4 * q + 4].reshape(-1)] == list(range(base + 64 * q, base + 64 * q + 64))


@pytest.mark.parametrize("b", BS)
def test_cover_without_the_tail(b, lib):
    """Static K1: every ngroups in the band, each with its own cg: the groups below min(end, ngroups) are exactly
    [0, ngroups), each once."""
    W = 16 * b
    for order, scr in ORDERS:
        cache = {}
        for cg0 in CGS:
            for ngroups in range(max(1, W * cg0 - BAND), W * cg0 + BAND + 1):
                cg = (ngroups + W - 1) // W
                if cg not in cache:
                    cache[cg] = o.groups(o.order_for(order, cg), scr, b, 16, cg).reshape(-1)
                    assert np.array_equal(np.sort(cache[cg]), np.arange(W * cg, dtype=np.uint64)), (order, scr, b, cg)
                g = cache[cg]
                read = g[g < ngroups]
                assert read.size == ngroups, (order, scr, b, ngroups)
                if ngroups in (W * cg0 - BAND, W * cg0 - 1, W * cg0, W * cg0 + 1, W * cg0 + BAND):
                    assert np.array_equal(np.sort(read), np.arange(ngroups, dtype=np.uint64)), (order, scr, b, ngroups)


@pytest.mark.parametrize("b", BS)
def test_static_part_with_the_tail(b, lib):
    """With the claimed tail the static part is groups [0, W cg_s), tiled by the walks of cg_s steps."""
    W = 16 * b
    ns = sorted({n for cg0 in CGS for n in (W * cg0 - BAND, W * cg0 - 1, W * cg0, W * cg0 + 1, W * cg0 + BAND)})
    splits = t.library_splits([(n, W) for n in ns])
    for ngroups, (cg_s, pool0, nchunks, _) in zip(ns, splits):
        assert cg_s % 4 == 0 and pool0 == W * cg_s <= ngroups
        for order, scr in ORDERS:
            g = o.groups(o.order_for(order, cg_s), scr, b, 16, cg_s)
            assert np.array_equal(np.sort(g.reshape(-1)), np.arange(pool0, dtype=np.uint64)), (order, scr, b, ngroups)


SIM = [(1, 31), (1, 33), (1, 40), (8, 32), (8, 33), (8, 34), (8, 35), (8, 40), (255, 32), (255, 33)]


@pytest.mark.parametrize("b,cg", SIM)
def test_kernel_path_without_the_tail(b, cg):
    """The loops of k_fixed_body, wave by wave: every wave executes k1_rounds(cg) barriers; every group of the batch is
    checksummed from its own two halves and stored once; nothing but the batch's groups is loaded from it, each half
    once (traffic 1.0)."""
    W = 16 * b
    S = m.round_steps()
    for order, scr in ORDERS:
        for nitems in sorted({2 * W * cg, 2 * W * cg - 1, 2 * W * cg - 2 * W + 2, 2 * W * cg - 2 * W + 1, 2 * W * cg - 9 * 16 * 2 - 3}):
            if nitems <= 0:
                continue
            r = o.simulate(order, scr, b, 16, nitems, tail=False)
            ngroups = (nitems + 1) // 2
            assert r["rounds"] == m.library_rounds([r["cg"]])[1][0] == (r["cg"] // S if r["cg"] >= 32 else 0)
            assert r["barriers"] == [r["rounds"]] * W, (order, scr, b, nitems)
            assert sorted(r["stored"]) == list(range(ngroups)) and set(r["stored"].values()) == {1}, (order, scr, b, nitems)
            halves = sorted(h for w in r["loaded"] for h in w)
            assert halves == [(gi, q) for gi in range(ngroups) for q in (0, 1)], (order, scr, b, nitems)


@pytest.mark.parametrize("b,cg", [(1, 40), (8, 40), (8, 41), (8, 127), (255, 40)])
def test_kernel_path_with_the_tail(b, cg):
    """The static part before the tail loop: k1_rounds(cg_s) barriers per wave; the loop leaves every wave at its last
    static pass with that pass's first three half-steps in the ring; static passes and left passes tile [0, W cg_s)."""
    W = 16 * b
    for order, scr in ORDERS:
        for nitems in (2 * W * cg, 2 * W * cg - 2 * W + 1):
            r = o.simulate(order, scr, b, 16, nitems, tail=True)
            cg_s, pool0 = r["cg"], r["limit"]
            assert cg_s >= 32 and r["run"] == order and pool0 == W * cg_s
            assert r["barriers"] == [cg_s // 4] * W
            covered = dict(r["stored"])
            loaded = sorted(h for w in r["loaded"] for h in w)
            for grp, ss, ring in r["left"]:
                assert ring[0] == (grp, 0) and ring[1] == (grp, 1) and ring[2] == (grp + ss, 0), (order, scr, grp, ring)
                for j in range(4):
                    covered[grp + j * ss] = covered.get(grp + j * ss, 0) + 1
            assert sorted(covered) == list(range(pool0)) and set(covered.values()) == {1}, (order, scr, b, nitems)
            # loaded so far: the stored groups whole, and of each left pass its first group and the next one's first half
            want = [(gi, q) for gi in r["stored"] for q in (0, 1)]
            want += [h for grp, ss, _ in r["left"] for h in ((grp, 0), (grp, 1), (grp + ss, 0))]
            assert loaded == sorted(want), (order, scr, b, nitems)
