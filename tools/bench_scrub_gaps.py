#!/usr/bin/env python3
"""crc32c_scrub_pages with and without CRC32C_SCRUB_GAPS, in one process, on
the pages tools/bench_scrub.py uses.

    python tools/bench_scrub_gaps.py [--pages 300] [--host-pages 30] [--repeats 10] [--warmup 2]
                                     [--out profiles/scrub_gaps_ab.jsonl]

Rows (bench.workload_config5: 1007 packed 4165-B images per 4 MiB wbuf, one
flipped bit in 1 % of the images; clean: the damage undone):
    device_damaged, device_clean   device-resident pages
    host_damaged, host_clean       the first --host-pages pages in pageable host
                                   memory
One sample is one whole scrub on a fresh copy of the page (restored outside the
timed region), wall clock around the synchronous call; the two settings
alternate sample by sample, medians of --repeats after --warmup.  Per setting
the row holds every sample's ms, the rounds, the flips, the entries of the
final list and the proven ones among them (kinds 1 and 4: the images a
read-back takes).  A clean page has no kind-4 entry and so no gap start: its
row also holds the spread of each setting's own samples, the margin the
difference of the two medians is held against.  Every row is a raw JSON line,
the last line is the summary.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pages", type=int, default=300)
    ap.add_argument("--host-pages", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scrub_gaps_ab.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from memcached_amd import _lib
    lib = _lib.lib
    # (the pages and the damage of tools/bench_scrub.py, seed for seed)
    (_base, nbytes_all, wbuf, _offs_p, n_all, _ok_p), _ok, _victims, _sb, _meta = \
        bench.workload_config5(argparse.Namespace(pages=args.pages), 0, 1)
    data, offs_all = bench._KEEP[-2], bench._KEEP[-1]
    damaged = data.clone()
    gen = torch.Generator(device="cuda").manual_seed(3)
    victims = torch.randperm(n_all, device="cuda", generator=gen)[: n_all // 100]
    pos = offs_all[victims] + 32 + torch.randint(0, 4165 - 32, (victims.numel(),), device="cuda", generator=gen)
    bit = torch.randint(0, 8, (victims.numel(),), device="cuda", generator=gen).to(torch.uint8)
    clean = damaged.clone()
    clean.view(-1)[pos] ^= (torch.ones_like(bit) << bit)
    st = torch.cuda.current_stream().cuda_stream
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def row(name, dev, source, nbytes, n):
        """source: the page's bytes to start every sample from (a device tensor)."""
        cap, fcap = 2 * n, n
        if dev:
            page = data.view(-1)[:nbytes]
            restore = lambda: page.copy_(source)  # noqa: E731
            new = lambda k, t: torch.empty(k, dtype=t, device="cuda")  # noqa: E731
            arrays = [new(cap, torch.int64), new(cap, torch.int32), new(cap, torch.uint8), new(fcap, torch.int64),
                      new(fcap, torch.int64), new(fcap, torch.uint8)]
            ptr, flag, stream = (lambda a: a.data_ptr()), _lib.CRC32C_DEVICE, st
            host = lambda a, k: a[:k].cpu().numpy()  # noqa: E731
        else:
            src = source.cpu().numpy()
            page = np.empty(nbytes, np.uint8)
            restore = lambda: np.copyto(page, src)  # noqa: E731
            arrays = [np.empty(cap, np.uint64), np.empty(cap, np.uint32), np.empty(cap, np.uint8),
                      np.empty(fcap, np.uint64), np.empty(fcap, np.uint64), np.empty(fcap, np.uint8)]
            ptr, flag, stream = (lambda a: a.ctypes.data), 0, None
            host = lambda a, k: a[:k]  # noqa: E731
        out = _lib.ScrubOut(*map(ptr, arrays[:3]), cap, *map(ptr, arrays[3:]), fcap)
        settings = [("off", _lib.ScrubOpts(flag, 0, 0, stream)),
                    ("gaps", _lib.ScrubOpts(flag | _lib.CRC32C_SCRUB_GAPS, 0, 0, stream))]
        ms, result = {k: [] for k, _ in settings}, {}
        for rep in range(args.warmup + args.repeats):
            for which, opts in settings:
                restore()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc = lib.crc32c_scrub_pages(ptr(page), nbytes, wbuf, ctypes.byref(opts), ctypes.byref(out))
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    ms[which].append(round((time.perf_counter() - t0) * 1e3, 4))
                _lib.check(rc)
                assert out.nflips <= fcap and out.nitems <= cap and out.complete == 1
                kind = host(arrays[2], out.nitems)
                result[which] = {"rounds": out.rounds, "nflips": out.nflips, "headers_repaired": out.headers_repaired,
                                 "items_repaired": out.items_repaired, "nitems": out.nitems,
                                 "proven": int(((kind == 1) | (kind == 4)).sum())}
        med = {k: round(statistics.median(v), 4) for k, v in ms.items()}
        rec = {"case": name, "bytes": nbytes, "ms": ms, "median_ms": med, "result": result,
               "gaps_minus_off_ms": round(med["gaps"] - med["off"], 4),
               "images_gained": result["gaps"]["proven"] - result["off"]["proven"],
               "spread_ms": {k: round(max(v) - min(v), 4) for k, v in ms.items()}}
        emit(rec)
        return rec

    rows = [row("device_damaged", True, damaged, nbytes_all, n_all), row("device_clean", True, clean, nbytes_all, n_all)]
    hp = min(args.host_pages, args.pages)
    hb, hn = hp * 16 * wbuf, hp * 16 * 1007
    rows += [row("host_damaged", False, damaged.view(-1)[:hb], hb, hn), row("host_clean", False, clean.view(-1)[:hb], hb, hn)]
    emit({"summary": True, "pages": args.pages, "host_pages": hp, "repeats": args.repeats,
          "median_ms": {r["case"]: r["median_ms"] for r in rows},
          "gaps_minus_off_ms": {r["case"]: r["gaps_minus_off_ms"] for r in rows},
          "spread_ms": {r["case"]: r["spread_ms"] for r in rows},
          "images_gained": {r["case"]: r["images_gained"] for r in rows},
          "rounds": {r["case"]: {k: v["rounds"] for k, v in r["result"].items()} for r in rows},
          "nflips": {r["case"]: {k: v["nflips"] for k, v in r["result"].items()} for r in rows}})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
