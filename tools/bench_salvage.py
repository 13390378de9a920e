#!/usr/bin/env python3
"""What crc32c_salvage_pages costs and recovers on device-resident config-5
pages (bench.workload_config5: 1007 packed 4165-B images per 4 MiB wbuf, one
flipped bit in 1 % of the images, a few hundred of which hit a header field).
One process, timed with device events; medians of --repeats calls after
--warmup.

    python tools/bench_salvage.py [--pages 300] [--repeats 10] [--out profiles/salvage.jsonl]

    1  crc32c_verify_pages alone
    2  verify_pages, then salvage_pages with its lists (nfound, scanned, ncand,
       and the share of the images the walk did not reach that came back; the
       offsets found in --check-wbufs damaged wbufs are compared with the
       prefiltering model of tests/salvage_model.py on the CPU)
    3  the same on the pages with the damage undone (tails only: what every
       clean compaction pays)
    4  salvage_pages with no lists: the whole buffer is scanned; the scan
       kernel's own time (crc32c_last_kernel_ms) as bytes per second

    python tools/bench_salvage.py --ab --lib /path/to/parent/libmcrc32c.so

times verify_pages alone in fresh child processes, this library and the
parent's alternating (as tools/keep_stamped_ab.py does), and holds the
difference of the medians against twice the spread of the parent's repeats.
Every sample is one raw JSON line; the last line is the summary.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pages(args):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from memcached_amd import _lib
    (base, nbytes, wbuf, _offs_p, n, _ok_p), _ok, _victims, _sb, _meta = \
        bench.workload_config5(argparse.Namespace(pages=args.pages), 0, 1)
    return torch, bench, _lib, bench._KEEP[-2], bench._KEEP[-1], base, nbytes, wbuf, n


def _timed(torch, fn, warmup, repeats):
    ms = []
    for rep in range(warmup + repeats):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if rep >= warmup:
            ms.append(round(e0.elapsed_time(e1), 4))
    return ms


def verify_child(args):
    torch, _bench, _lib, _data, _offs, base, nbytes, wbuf, n = _pages(args)
    lib = _lib.lib
    st = torch.cuda.current_stream().cuda_stream
    woffs = torch.empty(n, dtype=torch.int64, device="cuda")
    wok = torch.empty(n, dtype=torch.uint8, device="cuda")
    nitems, nbad = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def verify():
        _lib.check(lib.crc32c_verify_pages(base, nbytes, wbuf, woffs.data_ptr(), wok.data_ptr(), n,
                                           ctypes.byref(nitems), ctypes.byref(nbad), _lib.CRC32C_DEVICE, st))
    ms = _timed(torch, verify, args.warmup, args.repeats)
    print(json.dumps({"lib": args.which, "round": args.round, "case": "verify_pages", "pages": args.pages,
                      "items": int(nitems.value), "nbad": int(nbad.value), "ms": ms}), flush=True)


def ab(args, ap):
    if not args.lib or not os.path.exists(args.lib):
        ap.error("--lib: the parent library's path is required")
    lines = []
    for rnd in range(args.rounds):
        for which in ("parent", "this"):
            env = dict(os.environ)
            env.pop("MCRC_LIB", None)
            if which == "parent":
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
    ms = {"parent": [], "this": []}
    for ln in lines:
        rec = json.loads(ln)
        ms[rec["lib"]] += rec["ms"]
    med = {k: round(statistics.median(v), 4) for k, v in ms.items()}
    spread = round(max(ms["parent"]) - min(ms["parent"]), 4)
    lines.append(json.dumps({"summary": True, "case": "verify_pages_ab", "pages": args.pages,
                             "samples_per_lib": args.rounds * args.repeats, "median_ms": med,
                             "parent_spread_ms": spread, "this_minus_parent": round(med["this"] - med["parent"], 4),
                             "margin": round(2 * spread, 4),
                             "within_margin": med["this"] - med["parent"] <= 2 * spread}))
    print(lines[-1], flush=True)
    _write(args.out, lines, "a")
    return 0


def _write(path, lines, mode):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, mode) as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pages", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check-wbufs", type=int, default=6, help="damaged wbufs compared with the CPU model")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "salvage.jsonl"))
    ap.add_argument("--ab", action="store_true", help="verify_pages alone, this library against --lib")
    ap.add_argument("--lib", help="the parent commit's build of libmcrc32c.so")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--which", choices=["parent", "this"], help=argparse.SUPPRESS)
    ap.add_argument("--round", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.which:
        return verify_child(args)
    if args.ab:
        return ab(args, ap)

    torch, _bench, _lib, data, offs, base, nbytes, wbuf, n = _pages(args)
    import numpy as np
    from tests import salvage_model as sm
    lib = _lib.lib
    st = torch.cuda.current_stream().cuda_stream
    dev = _lib.CRC32C_DEVICE
    woffs = torch.empty(n, dtype=torch.int64, device="cuda")
    wok = torch.empty(n, dtype=torch.uint8, device="cuda")
    found = torch.empty(n, dtype=torch.int64, device="cuda")
    nitems, nbad = ctypes.c_uint64(0), ctypes.c_uint64(0)
    nfound, scanned, ncand = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    scan_ms = []

    def verify():
        _lib.check(lib.crc32c_verify_pages(base, nbytes, wbuf, woffs.data_ptr(), wok.data_ptr(), n,
                                           ctypes.byref(nitems), ctypes.byref(nbad), dev, st))

    def salvage(lists=True):
        nw = nitems.value if lists else 0
        _lib.check(lib.crc32c_salvage_pages(base, nbytes, wbuf, woffs.data_ptr() if nw else None,
                                            wok.data_ptr() if nw else None, nw, found.data_ptr(), n,
                                            ctypes.byref(nfound), ctypes.byref(scanned), ctypes.byref(ncand), dev, st))
        scan_ms.append(float(lib.crc32c_last_kernel_ms()))

    def both():
        verify()
        salvage()

    lines = []

    def case(name, fn, **extra):
        del scan_ms[:]
        ms = _timed(torch, fn, args.warmup, args.repeats)
        rec = {"case": name, "pages": args.pages, "ms": ms, "median_ms": round(statistics.median(ms), 4),
               "walked": int(nitems.value), "nbad": int(nbad.value), **extra}
        if scan_ms:
            rec.update(nfound=int(nfound.value), scanned=int(scanned.value), ncand=int(ncand.value),
                       scan_kernel_ms=round(statistics.median(scan_ms[args.warmup:]), 4))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        return rec

    r1 = case("1_verify_pages", verify)
    r2 = case("2_verify_then_salvage", both)
    unreached = n - r2["walked"]
    # the offsets found in a few damaged wbufs against the CPU model
    got = found[:r2["nfound"]].cpu().numpy()
    walked = woffs[:r2["walked"]].cpu().numpy()
    flags = wok[:r2["walked"]].cpu().numpy()
    short = [w for w, c in enumerate(np.bincount(walked // wbuf, minlength=nbytes // wbuf).tolist()) if c < 1007]
    checked = 0
    for w in short[:args.check_wbufs]:
        piece = data[w * wbuf:(w + 1) * wbuf].cpu().numpy()
        sel = walked // wbuf == w
        want = sm.salvage_fast(piece, wbuf, walked[sel] - w * wbuf, flags[sel])[0]
        mine = (got[got // wbuf == w] - w * wbuf).tolist()
        assert mine == want, (w, len(mine), len(want))
        checked += 1
    lines.append(json.dumps({"case": "2_recovered", "images_written": n, "walk_reached": r2["walked"],
                             "unreached": unreached, "nfound": r2["nfound"],
                             "recovered_share": round(r2["nfound"] / max(unreached, 1), 4),
                             "damaged_wbufs": len(short), "wbufs_checked_against_model": checked}))
    print(lines[-1], flush=True)

    r4 = case("4_salvage_no_lists", lambda: salvage(False))
    bps = r4["scanned"] / (r4["scan_kernel_ms"] * 1e-3)
    lines.append(json.dumps({"case": "4_scan_kernel", "scan_kernel_ms": r4["scan_kernel_ms"],
                             "read_bytes": r4["scanned"], "bytes_per_s": round(bps, 1),
                             "share_of_8TBps": round(bps / 8e12, 4)}))
    print(lines[-1], flush=True)

    # the damage undone (bench.workload_config5's generator replayed): clean pages, tails only
    gen = torch.Generator(device="cuda").manual_seed(3)
    victims = torch.randperm(n, device="cuda", generator=gen)[: n // 100]
    pos = offs[victims] + 32 + torch.randint(0, 4165 - 32, (victims.numel(),), device="cuda", generator=gen)
    bit = torch.randint(0, 8, (victims.numel(),), device="cuda", generator=gen).to(torch.uint8)
    data.view(-1)[pos] ^= (torch.ones_like(bit) << bit)
    verify()
    assert nitems.value == n and nbad.value == 0, "the damage was not undone"
    r3v = case("3_clean_verify_pages", verify)
    r3 = case("3_clean_verify_then_salvage", both)
    assert r3["nfound"] == 0
    lines.append(json.dumps({"summary": True, "pages": args.pages, "verify_ms": r1["median_ms"],
                             "verify_then_salvage_ms": r2["median_ms"], "clean_verify_ms": r3v["median_ms"],
                             "clean_verify_then_salvage_ms": r3["median_ms"],
                             "clean_salvage_share_of_verify": round(r3["median_ms"] / r3v["median_ms"] - 1, 4),
                             "no_lists_ms": r4["median_ms"], "recovered_share": round(r2["nfound"] / max(unreached, 1), 4)}))
    print(lines[-1], flush=True)
    _write(args.out, lines, "w")
    return 0


if __name__ == "__main__":
    sys.exit(main())
