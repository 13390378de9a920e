"""K1's order (memcached_amd/csrc/k_consts.h k1_walk / k1_group, the loops of
k_fixed_body in k_fixed.h) restated in Python, and the library's own mapping
read through tests/integration/k1_order_check.cpp, a stand-alone program over
k_consts.h built with -fsanitize=address,undefined.  Shared by
test_k1_order_model.py and test_gpu_k1_order.py."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

from . import k1_rounds_model as m
from . import k1_tail_model as t

RANGES, WINDOW_STEP, WINDOW_PASS = 0, 1, 2
PRIME = 65521
SRC = os.path.join(m.ROOT, "tests", "integration", "k1_order_check.cpp")


def scramble(i, n):
    return (i * PRIME) % n if n % PRIME else i


def order_for(order, cg):
    """Window orders only in launches with lockstep rounds."""
    return order if cg >= m.rounds_min_steps() else RANGES


def walk(order, scr, b, tt, nwg, wv, cg):
    """(first, sstep, pstep, rfirst, end) of wave slot tt of workgroup b."""
    whole, rem = cg - cg % 4, cg % 4
    if order == RANGES:
        first = scramble(b * wv + tt, nwg * wv) * cg
        return first, 1, 4, first + whole, first + cg
    base = (scramble(b, nwg) if scr else b) * wv * cg
    if order == WINDOW_PASS:
        rfirst = base + wv * whole + rem * tt
        return base + 4 * tt, 1, 4 * wv, rfirst, rfirst + rem
    return base + tt, wv, 4 * wv, base + wv * whole + tt, base + wv * cg


def groups(order, scr, nwg, wv, cg):
    """uint64 array [nwg, wv, cg]: the group wave (b, t) reads at step s = 4 q + j
    (the remainder's steps behind the passes'), written out per order."""
    b = np.arange(nwg, dtype=np.uint64)[:, None, None]
    tt = np.arange(wv, dtype=np.uint64)[None, :, None]
    s = np.arange(cg, dtype=np.uint64)[None, None, :]
    q, j = s // 4, s % 4
    Q, rem = cg // 4, cg % 4
    if order == RANGES:
        w = b * wv + tt
        W = nwg * wv
        r = (w * PRIME) % W if W % PRIME else w
        return (r * cg + s) + np.zeros((nwg, wv, cg), np.uint64)
    rb = (b * PRIME) % nwg if scr and nwg % PRIME else b
    base = rb * (wv * cg)
    if order == WINDOW_PASS:
        return np.where(q < Q, base + 4 * wv * q + 4 * tt + j, base + 4 * wv * Q + rem * tt + j)
    return base + wv * s + tt


def checksum(g):
    """Sum of group x (index + 1) mod 2^64 in (b, t, s) order, as the check program's."""
    flat = g.reshape(-1).astype(np.uint64)
    with np.errstate(over="ignore"):
        return int((flat * np.arange(1, flat.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))


@functools.lru_cache(maxsize=None)
def _exe():
    d = tempfile.mkdtemp(prefix="k1_order_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    out = os.path.join(d, "k1_order_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", m.CSRC, SRC, "-o", out], check=True)
    return out


def library(cases):
    """[(order that runs, rounds, checksum, perm ok, layout ok)] for (order, scramble, nwg, wv, cg) cases,
    from the sanitized check program (its exit status must be 0)."""
    cases = list(cases)
    out = []
    for i in range(0, len(cases), 200):
        args = [str(int(x)) for c in cases[i:i + 200] for x in c]
        r = subprocess.run([_exe()] + args, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        assert not re.search(r"runtime error|AddressSanitizer", r.stderr), r.stderr[-4000:]
        out += [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return out


def simulate(order, scr, nwg, wv, nitems, tail):
    """Every wave's path through k_fixed_body's static part, statement by
    statement, with its ring of four half-buffers, for a launch of nitems on
    nwg workgroups of wv waves.  Asserts that every step of a group inside the
    batch checksums that group's two halves, loaded from the batch.  Returns
    dict(cg, rounds, run, limit, barriers=[per wave, the tail's last one left
    out], loaded=[(group, half) loaded from the batch, per wave], stored={group:
    times stored}, left=[(group, step stride, ring) at the static part's end, per
    wave]).  With tail the static part is k1_tail_split's and ends before each
    wave's last pass, which is the tail loop's first chunk; the pool is not
    walked (k1_tail_model does that)."""
    W = nwg * wv
    ngroups = (nitems + 1) // 2
    if tail:
        (cg, pool0, _, _), = t.library_splits([(ngroups, W)])
    else:
        cg, pool0 = (ngroups + W - 1) // W, None
    S, (rounds,) = m.library_rounds([cg])
    run = order_for(order, cg)
    res = dict(cg=cg, rounds=rounds, run=run, limit=pool0, barriers=[], loaded=[], stored={}, left=[])
    stored = res["stored"]
    for b in range(nwg):
        for tt in range(wv):
            first, ss, ps, rfirst, end = walk(run, scr, b, tt, nwg, wv, cg)
            gend = min(end, ngroups)
            owed, nbar, loaded, ring = rounds, 0, [], [None] * 4

            def ldh(slot, gi, q):
                real = gi < gend
                ring[slot] = (gi if real else None, q)  # (None: the table image)
                if real:
                    loaded.append((gi, q))

            def step(cur, slots, a, b_):
                """step_even2 (slots 0, 1; refills 3, 0) or step_odd2 (2, 3; refills 1, 2)"""
                sa, sb = slots
                ldh((sa + 3) % 4, a, 1)
                first_half = ring[sa]
                ldh(sa, b_, 0)
                second_half = ring[sb]
                if 2 * cur < nitems:
                    assert first_half == (cur, 0) and second_half == (cur, 1), (b, tt, cur, first_half, second_half)
                    stored[cur] = stored.get(cur, 0) + 1

            grp = first
            if grp < ngroups:  # busy
                nsteps = (cg if run != RANGES else gend - grp) - (4 if tail else 0)
                nwhole = (nsteps + (4 if tail else 0)) & ~3
                ldh(0, grp, 0)
                ldh(1, grp, 1)
                ldh(2, grp + ss, 0)
                k = 0
                while k + 4 <= nsteps:
                    nxt = grp + ps if run == RANGES or k + 8 <= nwhole else rfirst
                    step(grp, (0, 1), grp + ss, grp + 2 * ss)
                    step(grp + ss, (2, 3), grp + 2 * ss, grp + 3 * ss)
                    step(grp + 2 * ss, (0, 1), grp + 3 * ss, nxt)
                    step(grp + 3 * ss, (2, 3), nxt, nxt + ss)
                    grp = nxt
                    if (k + 4) % S == 0 and owed:
                        nbar += 1
                        owed -= 1
                    k += 4
                while k + 2 <= nsteps:
                    step(grp, (0, 1), grp + ss, grp + 2 * ss)
                    step(grp + ss, (2, 3), grp + 2 * ss, grp + 3 * ss)
                    grp += 2 * ss
                    k += 2
                if nsteps & 1:
                    step(grp, (0, 1), grp + ss, grp + 2 * ss)
            nbar += owed  # the make-up loop
            res["barriers"].append(nbar)
            res["loaded"].append(loaded)
            res["left"].append((grp, ss, list(ring)))
    return res
