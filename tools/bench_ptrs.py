#!/usr/bin/env python3
"""Pointer batches against the offsets call they replace, per call and
synchronous (needs a gfx950 device).

    python tools/bench_ptrs.py --parent /path/to/parent/libmcrc32c.so

The yardstick is crc32c_batch of another build of the library, the parent
commit's (--parent; loaded beside this build in one process); without it the
yardstick is this build's own crc32c_batch and the record says so.  A run
alternates repetitions of its forms, --reps of each after one unrecorded
warm-up; a repetition is `calls` calls timed one by one, and counts as its
median.  Per form the record holds the repetitions' medians, their median and
their max - min.

  (a) io_batch   64 x 4133 B in one page-locked arena (the images 4165 B
                 apart): crc32c_batch over base + offsets against
                 crc32c_batch_ptrs over the same addresses.  The expected
                 difference is the per-span registry lookup, timed on the host
                 alone by tools/ptr_lookup.cpp (record "lookup").
  (b) chunks     64 x 512 KiB iovs spread over a 1 GiB page-locked arena:
                 crc32c_batch stages the windows between them; the pointer call
                 copies one DMA per span.  "ptrs_host_copy" is the same batch
                 with 1024 empty spans added, which puts the slot under the DMA
                 threshold (kPtrDmaMin): the host copies the spans instead.
  (c) pageable   64 and 8192 x 4133 B, every span a numpy array of its own,
                 against crc32c_batch over one contiguous pageable buffer of
                 the same bytes.

Appends one JSON line per run to profiles/ptr_batches.jsonl (--out).
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

try:  # GPU processes load torch (and its HIP runtime) before libmcrc32c.so
    import torch  # noqa: F401
except ImportError:
    pass

from memcached_amd import _lib  # noqa: E402
from tests import oracle  # noqa: E402

KiB, MiB, GiB = 1 << 10, 1 << 20, 1 << 30


def load_parent(path):
    """Another build's crc32c_batch, its symbols bound to itself."""
    lib = ctypes.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
    lib.crc32c_init()
    lib.crc32c_batch.restype, lib.crc32c_batch.argtypes = _lib.PROTOTYPES["crc32c_batch"]
    return lib


def rep_median_us(call, calls):
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        rc = call()
        t.append((time.perf_counter() - t0) * 1e6)
        assert rc == 0, rc
    return statistics.median(t)


def alternate(forms, calls, reps):
    """forms: name -> call.  One warm-up repetition of each, then reps of each in turn."""
    for call in forms.values():
        rep_median_us(call, max(2, calls // 4))
    meds = {name: [] for name in forms}
    for _ in range(reps):
        for name, call in forms.items():
            meds[name].append(rep_median_us(call, calls))
    return {name: dict(rep_medians_us=[round(x, 2) for x in m], median_us=round(statistics.median(m), 2),
                       spread_us=round(max(m) - min(m), 2)) for name, m in meds.items()}


def pinned(nbytes):
    p = _lib.lib.crc32c_host_alloc(nbytes)
    assert p, "crc32c_host_alloc failed"
    return p, np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(p))


def offsets_call(lib, base, nbytes, offs, length, out):
    sp = _lib.Spans(base, nbytes, offs.ctypes.data, 0, None, length, None, out.ctypes.data, offs.size)
    return lambda: lib.crc32c_batch(ctypes.byref(sp), 0, None)


def ptrs_call(ptrs, lens, length, out):
    b = _lib.PtrBatch(ptrs.ctypes.data, None if lens is None else lens.ctypes.data, length, None, out.ctypes.data,
                      ptrs.size)
    return lambda: _lib.lib.crc32c_batch_ptrs(ctypes.byref(b), None)


def lookup_cost():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "ptr_lookup")
        subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "memcached_amd", "csrc"),
                        os.path.join(ROOT, "tools", "ptr_lookup.cpp"), "-o", exe], check=True)
        return json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)


def run_io_batch(yard, reps, rng):
    n, length, pitch = 64, 4133, 4165
    p, arena = pinned(n * pitch)
    arena[:] = rng.integers(0, 256, arena.size, dtype=np.uint8)
    offs = np.arange(n, dtype=np.uint64) * pitch + 32
    want = oracle.batch(arena, offs, np.full(n, length))
    o1, o2 = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    res = alternate({"batch": offsets_call(yard, p, arena.size, offs, length, o1),
                     "ptrs": ptrs_call(offs + np.uint64(p), None, length, o2)}, 200, reps)
    assert (o1 == want).all() and (o2 == want).all()
    _lib.lib.crc32c_host_free(p)
    return res


def run_chunks(yard, reps, rng):
    n, length = 64, 512 * KiB
    p, arena = pinned(GiB)
    offs = np.arange(n, dtype=np.uint64) * (16 * MiB) + np.arange(n, dtype=np.uint64) % 16
    for o in offs:
        arena[int(o):int(o) + length] = rng.integers(0, 256, length, dtype=np.uint8)
    want = oracle.batch(arena, offs, np.full(n, length))
    o1, o2, o3 = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n + 1024, np.uint32)
    ptrs = offs + np.uint64(p)
    ptrs3 = np.concatenate((ptrs, np.zeros(1024, np.uint64)))
    lens3 = np.concatenate((np.full(n, length, np.uint32), np.zeros(1024, np.uint32)))
    res = alternate({"batch": offsets_call(yard, p, arena.size, offs, length, o1),
                     "ptrs": ptrs_call(ptrs, None, length, o2),
                     "ptrs_host_copy": ptrs_call(ptrs3, lens3, 0, o3)}, 5, reps)
    assert (o1 == want).all() and (o2 == want).all() and (o3[:n] == want).all() and (o3[n:] == 0).all()
    _lib.lib.crc32c_host_free(p)
    return res


def run_pageable(yard, reps, rng, n):
    length = 4133
    whole = rng.integers(0, 256, n * length, dtype=np.uint8)
    offs = np.arange(n, dtype=np.uint64) * length
    arrays = [whole[i * length:(i + 1) * length].copy() for i in range(n)]
    want = oracle.batch(whole, offs, np.full(n, length))
    o1, o2 = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    ptrs = np.array([a.ctypes.data for a in arrays], np.uint64)
    res = alternate({"batch": offsets_call(yard, whole.ctypes.data, whole.size, offs, length, o1),
                     "ptrs": ptrs_call(ptrs, None, length, o2)}, 100 if n <= 64 else 10, reps)
    assert (o1 == want).all() and (o2 == want).all()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="the parent commit's build of libmcrc32c.so: the yardstick's crc32c_batch")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", default="io_batch,chunks,pageable")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ptr_batches.jsonl"))
    args = ap.parse_args()
    assert _lib.lib.crc32c_gpu_count() >= 1, "needs a gfx950 device"
    yard = load_parent(args.parent) if args.parent else _lib.lib
    yardstick = "crc32c_batch of the parent build" if args.parent else "crc32c_batch of this build (no --parent)"
    rng = np.random.default_rng(2026)
    records = []
    for run in args.runs.split(","):
        if run == "io_batch":
            records.append(dict(run="io_batch", shape="64 x 4133 B, one page-locked arena", calls_per_rep=200,
                                forms=run_io_batch(yard, args.reps, rng), lookup=lookup_cost()))
        elif run == "chunks":
            records.append(dict(run="chunks", shape="64 x 512 KiB over a 1 GiB page-locked arena", calls_per_rep=5,
                                forms=run_chunks(yard, args.reps, rng)))
        elif run == "pageable":
            for n in (64, 8192):
                records.append(dict(run=f"pageable_{n}", shape=f"{n} x 4133 B pageable, one array per span",
                                    calls_per_rep=100 if n <= 64 else 10, forms=run_pageable(yard, args.reps, rng, n)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for r in records:
            r.update(yardstick=yardstick, reps=args.reps, unit="us per call, median of a repetition's calls")
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
