#!/usr/bin/env python3
"""crc32c_scrub_pages with and without CRC32C_SCRUB_BYTES, in one process, on
the pages tools/bench_scrub.py uses with byte damage added.

    python tools/bench_scrub_bytes.py [--pages 300] [--host-pages 30] [--repeats 10] [--warmup 2]
                                      [--out profiles/scrub_bytes.jsonl]

Rows (bench.workload_config5: 1007 packed 4165-B images per 4 MiB wbuf, one
flipped bit in 1 % of the images; byte damage: every tenth of those has a
second bit of the same byte inverted; clean: the damage undone):
    device_bytes, device_bits, device_clean   device-resident pages
    host_bytes, host_clean                    the first --host-pages pages in
                                              pageable host memory
One sample is one whole scrub on a fresh copy of the page (restored outside the
timed region), wall clock around the synchronous call; the settings -- off,
bytes, gaps, gaps_bytes -- alternate sample by sample, medians of --repeats
after --warmup.  Per setting the row holds every sample's ms, the rounds, the
flips (bits), the entries of the final list and the images lost: the page's
images that are not proven (kinds 1 and 4) in the final list.  ``device_bits``
and the clean rows have nothing for the byte stage to repair: there the bit
costs its one search per final round (bits) or nothing (clean: an empty item
list), and each setting's own spread is the margin its median is held against.
Every row is a raw JSON line, the last line is the summary.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scrub_bytes.jsonl"))
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
    bits = data.clone()
    gen = torch.Generator(device="cuda").manual_seed(3)
    victims = torch.randperm(n_all, device="cuda", generator=gen)[: n_all // 100]
    pos = offs_all[victims] + 32 + torch.randint(0, 4165 - 32, (victims.numel(),), device="cuda", generator=gen)
    bit = torch.randint(0, 8, (victims.numel(),), device="cuda", generator=gen).to(torch.uint8)
    clean = bits.clone()
    clean.view(-1)[pos] ^= (torch.ones_like(bit) << bit)
    # byte damage: every tenth damaged image gets a second bit of the same byte, where that byte lies behind the
    # 48-byte header (no length bit there); the others keep their single bit
    tenth = torch.arange(0, victims.numel(), 10, device="cuda")
    tenth = tenth[(pos[tenth] - offs_all[victims[tenth]]) >= 48]
    byted = bits.clone()
    byted.view(-1)[pos[tenth]] ^= (torch.ones_like(bit[tenth]) << ((bit[tenth] + 3) % 8))
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
        G, B = _lib.CRC32C_SCRUB_GAPS, _lib.CRC32C_SCRUB_BYTES
        settings = [(k, _lib.ScrubOpts(flag | m, 0, 0, stream))
                    for k, m in (("off", 0), ("bytes", B), ("gaps", G), ("gaps_bytes", G | B))]
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
                by = host(arrays[5], out.nflips)
                proven = int(((kind == 1) | (kind == 4)).sum())
                result[which] = {"rounds": out.rounds, "nflips": out.nflips, "headers_repaired": out.headers_repaired,
                                 "items_repaired": out.items_repaired, "nitems": out.nitems, "proven": proven,
                                 "lost": n - proven, "by_byte_flips": int((by == _lib.CRC32C_SCRUB_BY_BYTE).sum())}
        med = {k: round(statistics.median(v), 4) for k, v in ms.items()}
        rec = {"case": name, "bytes": nbytes, "images": n, "ms": ms, "median_ms": med, "result": result,
               "bytes_minus_off_ms": round(med["bytes"] - med["off"], 4),
               "gaps_bytes_minus_gaps_ms": round(med["gaps_bytes"] - med["gaps"], 4),
               "lost": {k: v["lost"] for k, v in result.items()},
               "spread_ms": {k: round(max(v) - min(v), 4) for k, v in ms.items()}}
        emit(rec)
        return rec

    rows = [row("device_bytes", True, byted, nbytes_all, n_all), row("device_bits", True, bits, nbytes_all, n_all),
            row("device_clean", True, clean, nbytes_all, n_all)]
    hp = min(args.host_pages, args.pages)
    hb, hn = hp * 16 * wbuf, hp * 16 * 1007
    rows += [row("host_bytes", False, byted.view(-1)[:hb], hb, hn), row("host_clean", False, clean.view(-1)[:hb], hb, hn)]
    emit({"summary": True, "pages": args.pages, "host_pages": hp, "repeats": args.repeats,
          "byte_damaged_images": int(tenth.numel()),
          "median_ms": {r["case"]: r["median_ms"] for r in rows},
          "bytes_minus_off_ms": {r["case"]: r["bytes_minus_off_ms"] for r in rows},
          "gaps_bytes_minus_gaps_ms": {r["case"]: r["gaps_bytes_minus_gaps_ms"] for r in rows},
          "spread_ms": {r["case"]: r["spread_ms"] for r in rows},
          "lost": {r["case"]: r["lost"] for r in rows},
          "rounds": {r["case"]: {k: v["rounds"] for k, v in r["result"].items()} for r in rows},
          "nflips": {r["case"]: {k: v["nflips"] for k, v in r["result"].items()} for r in rows}})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
