"""K1's claimed tail (memcached_amd/csrc/k_consts.h k1_tail_split, k_fixed.h
"The claimed tail", shim_launch.h k1_ctl) restated in Python around the
library's own split, read through a small host program compiled against
k_consts.h.  Shared by test_k1_tail_model.py and test_gpu_k1_tail.py."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

from . import k1_rounds_model as m

_PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "k_consts.h"
// prints the constants, then per (ngroups, W) pair of arguments: cg_s pool0 nchunks and the 16 sub-pools' chunk counts
int main(int argc, char **argv) {
    using namespace mcrc_dev;
    printf("%u %u %u %u %u\n", (unsigned)kK1TailShift, (unsigned)kK1TailSteps, (unsigned)kK1TailPools,
           (unsigned)kK1TailFloorSteps, (unsigned)kK1TailMinSteps);
    for (int i = 1; i + 1 < argc; i += 2) {
        const K1Tail t = k1_tail_split(strtoull(argv[i], nullptr, 10), strtoull(argv[i + 1], nullptr, 10));
        printf("%llu %llu %llu", (unsigned long long)t.cg_s, (unsigned long long)t.pool0, (unsigned long long)t.nchunks);
        for (uint32_t p = 0; p < kK1TailPools; ++p) printf(" %llu", (unsigned long long)k1_tail_pool_chunks(t.nchunks, p));
        printf("\n");
    }
    return 0;
}
"""


@functools.lru_cache(maxsize=None)
def _exe():
    d = tempfile.mkdtemp(prefix="k1_tail_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    src, out = os.path.join(d, "k1_tail.cpp"), os.path.join(d, "k1_tail")
    with open(src, "w") as f:
        f.write(_PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", m.CSRC, src, "-o", out], check=True)
    return out


def _run(pairs):
    args = [str(x) for p in pairs for x in p]
    r = subprocess.run([_exe()] + args, capture_output=True, text=True, check=True)
    return [[int(x) for x in line.split()] for line in r.stdout.splitlines()]


@functools.lru_cache(maxsize=None)
def consts():
    """dict(shift, steps, pools, floor, default_min) as k_consts.h has them."""
    return dict(zip(("shift", "steps", "pools", "floor", "default_min"), _run([])[0]))


def library_splits(pairs):
    """[(cg_s, pool0, nchunks, [chunks of sub-pool t])] for (ngroups, W) pairs."""
    pairs = list(pairs)
    out = []
    for i in range(0, len(pairs), 1000):
        out += [(r[0], r[1], r[2], r[3:]) for r in _run(pairs[i:i + 1000])[1:]]
    return out


def geometry(nitems, cus):
    """(W, ngroups, cg) of a K1 launch."""
    W = m.grid_for(cus, nitems) * 16
    ngroups = (nitems + 1) // 2
    return W, ngroups, (ngroups + W - 1) // W


def tail_on(nitems, cus, min_steps):
    """The host's decision (k1_ctl, a stream with a slot): the tail runs from min_steps steps per wave on."""
    return geometry(nitems, cus)[2] >= min_steps


def static_ranges(W, cg_s):
    """The static part's range per wave, in launch order: K1's scrambled deal of full ranges."""
    order = [(w * 65521) % W if W % 65521 else w for w in range(W)]
    return [(r * cg_s, (r + 1) * cg_s) for r in order]


def chunks(pool0, nchunks, ngroups):
    T = consts()["steps"]
    return [(pool0 + c * T, min(pool0 + (c + 1) * T, ngroups)) for c in range(nchunks)]


def wave_barriers(cg_s, S, rounds):
    """One wave's barriers on the tail path of k_fixed_body, counted where they
    execute: the 4-step loop runs the range but its last pass, the make-up loop
    pays what is still owed, the tail loop has none, one more ends the launch."""
    owed = rounds
    n = 0
    k = 0
    while k + 4 <= cg_s - 4:
        if (k + 4) % S == 0 and owed:
            n += 1
            owed -= 1
        k += 4
    while owed:
        n += 1
        owed -= 1
    return n + 1
