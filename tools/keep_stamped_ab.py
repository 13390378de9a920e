#!/usr/bin/env python3
"""Same-run A/B of the keep-stamped stamp and crc32c_stamp_pages against
another build of libmcrc32c.so (the parent commit's), on device-resident
config-5 pages (bench.workload_config5: 1007 packed 4165-B images per 4 MiB
wbuf), timed with device events after a warm-up.

    python tools/keep_stamped_ab.py --lib /path/to/parent/libmcrc32c.so \
        [--pages 300] [--repeats 5] [--rounds 3] [--out profiles/keep_stamped_ab.jsonl]

The driver starts one fresh child process per library and round, alternating
the two libraries (a library is chosen when memcached_amd._lib is imported, so
each child holds one).  Cases:

    other library   a  stamp_items            b  verify_items
    this library    c  stamp_items and verify_items (the old paths, unchanged?)
                    d  keep-stamped, all images fresh     (held against a)
                    e  keep-stamped, all images carried   (held against b)
                    f  keep-stamped, every other image fresh
                    g  stamp_pages against stamp_items with given offsets

Every sample is one raw JSON line; the last line is the summary: medians,
the run-to-run spread (max - min) of a and b, and d - a and e - b against a
margin of twice that spread.  A child that fails stops the run: nothing more
is started on the GPU after it.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(args):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from memcached_amd import _lib
    lib = _lib.lib
    (base, nbytes, wbuf, offs_p, n, ok_p), ok, _victims, _span_bytes, _meta = \
        bench.workload_config5(argparse.Namespace(pages=args.pages), 0, 1)
    data, offs = bench._KEEP[-2], bench._KEEP[-1]
    nwb = nbytes // wbuf
    exptime = data.view(nwb, wbuf)[:, :1007 * 4165].view(nwb, 1007, 4165)[..., 28:32]
    nbad = ctypes.c_uint64(0)
    nitems = ctypes.c_uint64(0)
    st = torch.cuda.current_stream().cuda_stream
    dev = _lib.CRC32C_DEVICE
    keep = getattr(_lib, "CRC32C_KEEP_STAMPED", 0)

    def stamp(flags=0):
        _lib.check(lib.crc32c_stamp_items(base, nbytes, wbuf, offs_p, n, ok_p, ctypes.byref(nbad), dev | flags, st))

    def verify():
        _lib.check(lib.crc32c_verify_items(base, nbytes, wbuf, offs_p, n, ok_p, ctypes.byref(nbad), dev, st))

    woffs = torch.empty(n, dtype=torch.int64, device="cuda")

    def stamp_pages(flags=0):
        _lib.check(lib.crc32c_stamp_pages(base, nbytes, wbuf, woffs.data_ptr(), ok_p, n, ctypes.byref(nitems),
                                          ctypes.byref(nbad), dev | flags, st))

    def fresh(step):
        exptime[:, ::step] = 0

    def timed(case, fn, prep=None):
        ms = []
        for rep in range(args.warmup + args.repeats):
            if prep:
                prep()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                ms.append(round(e0.elapsed_time(e1), 4))
        print(json.dumps({"lib": args.which, "round": args.round, "case": case, "pages": args.pages, "items": n,
                          "ms": ms, "nbad": int(nbad.value)}), flush=True)

    # Every image carries its CRC after this (the generator's flipped data
    # bits are covered too; the few flips that hit a header field leave
    # malformed images, which every case counts in nbad alike, and a few
    # images whose damaged length makes them overlap their neighbours'
    # exptime, whose verdict depends on the order of the stamps -- the
    # documented overlap case).  The plain
    # stamps get the same preparation as case d -- exptime zeroed before every
    # repeat -- so that all of them start from the same cache state (the
    # zeroing leaves dirty sectors behind that are written back while the next
    # kernel streams).
    stamp()
    nmal = nbad.value
    if args.which == "other":
        timed("a_stamp_items", stamp, lambda: fresh(1))
        timed("b_verify_items", verify)
        return
    timed("c_stamp_items", stamp, lambda: fresh(1))
    timed("c_verify_items", verify)
    timed("d_keep_all_fresh", lambda: stamp(keep), lambda: fresh(1))
    assert nbad.value == nmal and int((ok == 1).sum()) == n - nmal
    timed("e_keep_all_carried", lambda: stamp(keep))
    assert nbad.value >= nmal and int((ok == 2).sum()) == n - nbad.value
    timed("f_keep_half_fresh", lambda: stamp(keep), lambda: fresh(2))
    assert nbad.value >= nmal and int((ok == 0).sum()) == nbad.value and int((ok == 1).sum()) >= nwb * 504 - nmal
    timed("g_stamp_pages", stamp_pages, lambda: fresh(1))
    timed("g_stamp_items_given_offsets", stamp, lambda: fresh(1))
    timed("g_stamp_pages_keep_all_carried", lambda: stamp_pages(keep))
    assert int((ok == 2).sum()) == nitems.value - nbad.value


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="the other build of libmcrc32c.so (the parent commit's)")
    ap.add_argument("--pages", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keep_stamped_ab.jsonl"))
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--which", choices=["other", "this"], help=argparse.SUPPRESS)
    ap.add_argument("--round", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.which:
        return child(args)
    if not args.lib or not os.path.exists(args.lib):
        ap.error("--lib: the other library's path is required")
    lines = []
    for rnd in range(args.rounds):
        for which in ("other", "this"):
            env = dict(os.environ)
            env.pop("MCRC_LIB", None)
            if which == "other":
                env["MCRC_LIB"] = os.path.abspath(args.lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--which", which, "--round", str(rnd), "--pages",
                   str(args.pages), "--repeats", str(args.repeats), "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
            got = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            lines += got
            print("\n".join(got), flush=True)
            if r.returncode != 0:  # nothing more on the GPU after a failure
                sys.stderr.write(r.stdout + r.stderr)
                return r.returncode or 1
    ms = {}
    for ln in lines:
        rec = json.loads(ln)
        ms.setdefault(rec["case"], []).extend(rec["ms"])
    med = {k: round(statistics.median(v), 4) for k, v in ms.items()}
    spread = {k: round(max(ms[k]) - min(ms[k]), 4) for k in ("a_stamp_items", "b_verify_items")}
    summary = {"summary": True, "pages": args.pages, "samples_per_case": args.rounds * args.repeats, "median_ms": med,
               "min_ms": {k: min(v) for k, v in ms.items()}, "max_ms": {k: max(v) for k, v in ms.items()},
               "spread_ms": spread,
               "c_minus_a": round(med["c_stamp_items"] - med["a_stamp_items"], 4),
               "c_minus_b": round(med["c_verify_items"] - med["b_verify_items"], 4),
               "d_minus_a": round(med["d_keep_all_fresh"] - med["a_stamp_items"], 4),
               "d_margin": round(2 * spread["a_stamp_items"], 4),
               "e_minus_b": round(med["e_keep_all_carried"] - med["b_verify_items"], 4),
               "e_margin": round(2 * spread["b_verify_items"], 4),
               "g_pages_minus_items": round(med["g_stamp_pages"] - med["g_stamp_items_given_offsets"], 4)}
    lines.append(json.dumps(summary))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
