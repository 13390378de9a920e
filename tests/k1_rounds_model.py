"""K1's range split and lockstep rounds (memcached_amd/csrc/k_fixed.h,
k_consts.h, host_route.h grid_for) restated in Python, and the library's own
k1_rounds / kK1RoundSteps read through a small host program compiled against
k_consts.h.  Shared by test_k1_rounds_model.py and test_gpu_k1_lockstep.py."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "memcached_amd", "csrc")

_PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "k_consts.h"
// argv: cg values; prints kK1RoundSteps and kK1RoundsMinSteps, then k1_rounds(cg, kK1RoundSteps) per argument
int main(int argc, char **argv) {
    printf("%u %u\n", (unsigned)mcrc_dev::kK1RoundSteps, (unsigned)mcrc_dev::kK1RoundsMinSteps);
    for (int i = 1; i < argc; ++i)
        printf("%llu\n", (unsigned long long)mcrc_dev::k1_rounds(strtoull(argv[i], nullptr, 10), mcrc_dev::kK1RoundSteps));
    return 0;
}
"""


@functools.lru_cache(maxsize=None)
def _exe():
    d = tempfile.mkdtemp(prefix="k1_rounds_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    src, out = os.path.join(d, "k1_rounds.cpp"), os.path.join(d, "k1_rounds")
    with open(src, "w") as f:
        f.write(_PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, src, "-o", out], check=True)
    return out


def library_rounds(cgs):
    """(kK1RoundSteps, [k1_rounds(cg, kK1RoundSteps) for cg in cgs]) as k_consts.h computes them."""
    cgs = list(cgs)
    vals = []
    for i in range(0, max(len(cgs), 1), 2000):
        r = subprocess.run([_exe()] + [str(c) for c in cgs[i:i + 2000]], capture_output=True, text=True, check=True)
        lines = [int(x) for x in r.stdout.split()]
        steps, vals = lines[0], vals + lines[2:]
    return steps, vals


def round_steps():
    return library_rounds([])[0]


def rounds_min_steps():
    """kK1RoundsMinSteps: launches of fewer steps per wave run without rounds."""
    r = subprocess.run([_exe()], capture_output=True, text=True, check=True)
    return int(r.stdout.split()[1])


def grid_for(cus, n):
    return max(1, min((n + 31) // 32, cus))


def split(nitems, cus):
    """K1's ranges: (cg, [(first group, end group) per wave, in launch order])."""
    gstep = grid_for(cus, nitems) * 16
    ngroups = (nitems + 1) // 2
    cg = (ngroups + gstep - 1) // gstep
    ranges = []
    for w in range(gstep):
        grp = (w * 65521) % gstep if gstep % 65521 else w
        ranges.append((grp * cg, min((grp + 1) * cg, ngroups)))
    return cg, ranges


def walk(g0, g1, ngroups, cg, S, rounds):
    """One wave's path through k_fixed_body, statement by statement; every
    s_barrier it executes is counted where it executes, not derived from the
    counter the kernel keeps.  Returns (barriers executed in the 4-step loop,
    barriers executed in the make-up loop, round ends the 4-step loop passed,
    steps run per loop): `passed` counts every pass that ends a round, whether
    or not the kernel's `&& owed` let the wave arrive there."""
    owed = rounds
    in_loop = makeup = passed = 0
    loops = [0, 0, 0]
    if g0 < ngroups:  # (busy)
        nsteps = g1 - g0
        k = 0
        while k + 4 <= nsteps:
            if (k + 4) % S == 0:
                passed += 1
                if owed:
                    in_loop += 1  # k1_round_barrier()
                    owed -= 1
            k += 4
            loops[0] += 4
        while k + 2 <= nsteps:
            k += 2
            loops[1] += 2
        if nsteps & 1:
            loops[2] += 1
    while owed:
        makeup += 1  # k1_round_barrier()
        owed -= 1
    return in_loop, makeup, passed, loops
