#!/usr/bin/env python3
"""crc32c_repair_bytes against crc32c_repair_items on the same list, in one
process: device-resident config-5 pages with the bench's damage
(bench.workload_config5: 1007 packed 4165-B images per 4 MiB wbuf, one flipped
bit in 1 % of the images), the list of crc32c_recover_pages' entries with
kind == 0 && lens != 0, and the two calls alternating sample by sample with
CRC32C_LOCATE_ONLY (every sample sees the same damage).  Medians of --repeats
after --warmup; every sample is in a raw JSON line, the last line is the
summary.

    python tools/bench_repair_bytes.py [--pages 300] [--repeats 10] [--out profiles/repair_bytes.jsonl]

Rows:
    single_bit   the bench's damage: both calls locate every image
    byte_mask    a second bit of the same byte inverted in every damaged image
                 (on the device, by the position the first row located):
                 crc32c_repair_items locates none of them and still searches
                 every step, crc32c_repair_bytes locates them all
Per row and call: the call's time (device events) and the search kernel's
(crc32c_last_kernel_ms), with their spreads (max - min).  The yardstick is
crc32c_repair_items in the same run, never a stored figure.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pages", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repair_bytes.jsonl"))
    args = ap.parse_args()

    sys.path.insert(0, ROOT)
    import torch
    import bench
    from memcached_amd import _lib
    (base, nbytes, wbuf, _offs_p, n, _ok_p), _ok, _victims, _sb, _meta = \
        bench.workload_config5(argparse.Namespace(pages=args.pages), 0, 1)
    data = bench._KEEP[-2]
    lib = _lib.lib
    st = torch.cuda.current_stream().cuda_stream
    u64 = ctypes.c_uint64
    cap = 2 * n
    moffs = torch.empty(cap, dtype=torch.int64, device="cuda")
    mlens = torch.empty(cap, dtype=torch.int32, device="cuda")
    mkind = torch.empty(cap, dtype=torch.uint8, device="cuda")
    rok = torch.empty(cap, dtype=torch.uint8, device="cuda")
    rpos = torch.empty(cap, dtype=torch.int64, device="cuda")
    rmask = torch.empty(cap, dtype=torch.uint8, device="cuda")
    counts = [u64(0) for _ in range(5)]
    nrep, nbad = u64(0), u64(0)
    opts = _lib.BytesOpts(_lib.CRC32C_DEVICE | _lib.CRC32C_LOCATE_ONLY, 0, st)
    out = _lib.BytesOut(rok.data_ptr(), rpos.data_ptr(), rmask.data_ptr(), 0, 0)

    def bad_list():
        _lib.check(lib.crc32c_recover_pages(base, nbytes, wbuf, moffs.data_ptr(), mlens.data_ptr(), mkind.data_ptr(), cap,
                                            *map(ctypes.byref, counts), _lib.CRC32C_DEVICE, st))
        k = counts[0].value
        return moffs[:k][(mkind[:k] == 0) & (mlens[:k] != 0)].contiguous()

    def items(todo):
        _lib.check(lib.crc32c_repair_items(base, nbytes, wbuf, todo.data_ptr(), todo.numel(), 0, rok.data_ptr(),
                                           rpos.data_ptr(), ctypes.byref(nrep), ctypes.byref(nbad),
                                           _lib.CRC32C_DEVICE | _lib.CRC32C_LOCATE_ONLY, st))
        return nrep.value

    def bytes_(todo):
        _lib.check(lib.crc32c_repair_bytes(base, nbytes, wbuf, todo.data_ptr(), todo.numel(), ctypes.byref(opts),
                                           ctypes.byref(out)))
        return out.nrepaired

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        got = fn()
        e1.record()
        e1.synchronize()
        return round(e0.elapsed_time(e1), 4), round(float(lib.crc32c_last_kernel_ms()), 4), got

    def row(case, todo):
        ms = {"items_call": [], "items_search": [], "bytes_call": [], "bytes_search": []}
        for rep in range(args.warmup + args.repeats):
            a, ak, ia = timed(lambda: items(todo))
            b, bk, ib = timed(lambda: bytes_(todo))
            if rep >= args.warmup:
                for key, v in zip(ms, (a, ak, b, bk)):
                    ms[key].append(v)
        rec = {"case": case, "pages": args.pages, "given": todo.numel(), "items_located": ia, "bytes_located": ib,
               "ms": ms, "median_ms": {k: round(statistics.median(v), 4) for k, v in ms.items()},
               "spread_ms": {k: round(max(v) - min(v), 4) for k, v in ms.items()}}
        m = rec["median_ms"]
        rec["bytes_over_items"] = {"call": round(m["bytes_call"] / m["items_call"], 4),
                                   "search": round(m["bytes_search"] / m["items_search"], 4)}
        print(json.dumps(rec), flush=True)
        return rec

    todo = bad_list()
    rows = [row("single_bit", todo)]
    assert rows[0]["items_located"] == rows[0]["bytes_located"]

    # a second bit of the same byte, two places up (never a length bit of bytes 38 / 39 but from bits 7 / 6,
    # which such an image would show as not located)
    items(todo)
    torch.cuda.synchronize()
    k = todo.numel()
    hit = rok[:k] == _lib.CRC32C_ITEM_REPAIRED
    at = (todo + rpos[:k] // 8)[hit]
    extra = (1 << ((rpos[:k] % 8 + 2) % 8))[hit].to(torch.uint8)
    flat = data.view(-1)
    flat[at] = flat[at] ^ extra
    torch.cuda.synchronize()
    todo2 = bad_list()
    rows.append(row("byte_mask", todo2))

    rows.append({"summary": True, "pages": args.pages, "repeats": args.repeats,
                 **{r["case"]: {"median_ms": r["median_ms"], "spread_ms": r["spread_ms"],
                                "bytes_over_items": r["bytes_over_items"], "given": r["given"],
                                "items_located": r["items_located"], "bytes_located": r["bytes_located"]}
                    for r in rows}})
    print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(json.dumps(r) for r in rows) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
