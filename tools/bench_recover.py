#!/usr/bin/env python3
"""crc32c_recover_pages against the two calls it fuses, crc32c_verify_pages
followed by crc32c_salvage_pages, in one process.  The two flows alternate
sample by sample; medians of --repeats after --warmup; every sample is in a raw
JSON line, the last line is the summary.

    python tools/bench_recover.py [--pages 300] [--repeats 10] [--out profiles/recover.jsonl]

Rows:
    device_damaged   device-resident config-5 pages (bench.workload_config5: 1007
                     packed 4165-B images per 4 MiB wbuf, one flipped bit in 1 %
                     of the images), timed with device events
    device_clean     the same pages with the damage undone (tails only: what
                     every clean compaction pays)
    host_1, host_16  a page-locked host buffer (crc32c_host_alloc) of 1 and of
                     16 clean wbufs, one header bit flipped in one wbuf, timed
                     on the host clock (the calls return when the results are
                     in host memory)

The yardstick is the two-call flow.  A row counts as slower when the fused
median exceeds the two-call median by more than twice the spread (max - min)
of the two-call samples, the margin of tools/bench_salvage.py --ab.  Both flows'
counts are compared on every row.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pages", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recover.jsonl"))
    args = ap.parse_args()

    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench
    from memcached_amd import _lib
    (base, nbytes, wbuf, _offs_p, n, _ok_p), _ok, _victims, _sb, _meta = \
        bench.workload_config5(argparse.Namespace(pages=args.pages), 0, 1)
    data, offs = bench._KEEP[-2], bench._KEEP[-1]
    lib = _lib.lib
    st = torch.cuda.current_stream().cuda_stream
    u64 = ctypes.c_uint64
    lines = []

    def flows(base, nbytes, cap, flags, stream, arrays):
        """(two, fused, counts): the two flows over one buffer and what each last reported."""
        woffs, wok, found, moffs, mlens, mkind = arrays
        c2 = [u64(0) for _ in range(5)]  # nitems, nbad, nfound, scanned, ncand
        c1 = [u64(0) for _ in range(5)]  # nitems, nbad, nsalvaged, scanned, ncand
        r2, r1 = [ctypes.byref(c) for c in c2], [ctypes.byref(c) for c in c1]

        def two():
            _lib.check(lib.crc32c_verify_pages(base, nbytes, wbuf, woffs, wok, cap, r2[0], r2[1], flags, stream))
            _lib.check(lib.crc32c_salvage_pages(base, nbytes, wbuf, woffs, wok, c2[0].value, found, cap, r2[2], r2[3],
                                                r2[4], flags, stream))

        def fused():
            _lib.check(lib.crc32c_recover_pages(base, nbytes, wbuf, moffs, mlens, mkind, 2 * cap, *r1, flags, stream))

        def counts():
            a, b = [c.value for c in c2], [c.value for c in c1]
            assert (a[0] + a[2], a[1], a[2], a[3], a[4]) == tuple(b), (a, b)
            return dict(nitems=b[0], nbad=b[1], nsalvaged=b[2], scanned=b[3], ncand=b[4])
        return two, fused, counts

    def row(name, two, fused, counts, device):
        ms = {"two_calls": [], "fused": []}
        for rep in range(args.warmup + args.repeats):
            for which, fn in (("two_calls", two), ("fused", fused)):
                torch.cuda.synchronize()
                if device:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    t = e0.elapsed_time(e1)
                else:
                    t0 = time.perf_counter()
                    fn()
                    t = (time.perf_counter() - t0) * 1e3
                if rep >= args.warmup:
                    ms[which].append(round(t, 4))
        med = {k: round(statistics.median(v), 4) for k, v in ms.items()}
        spread = round(max(ms["two_calls"]) - min(ms["two_calls"]), 4)
        rec = {"case": name, "ms": ms, "median_ms": med, "two_calls_spread_ms": spread,
               "fused_minus_two_calls": round(med["fused"] - med["two_calls"], 4), "margin": round(2 * spread, 4),
               "slower": med["fused"] - med["two_calls"] > 2 * spread, **counts()}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        return rec

    # device-resident pages, damaged and clean
    t = [torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda"),
         torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(2 * n, dtype=torch.int64, device="cuda"),
         torch.empty(2 * n, dtype=torch.int32, device="cuda"), torch.empty(2 * n, dtype=torch.uint8, device="cuda")]
    dev_flows = flows(base, nbytes, n, _lib.CRC32C_DEVICE, st, [x.data_ptr() for x in t])
    rows = [row("device_damaged", *dev_flows, True)]
    # the damage undone (bench.workload_config5's generator replayed, as tools/bench_salvage.py does)
    gen = torch.Generator(device="cuda").manual_seed(3)
    victims = torch.randperm(n, device="cuda", generator=gen)[: n // 100]
    pos = offs[victims] + 32 + torch.randint(0, 4165 - 32, (victims.numel(),), device="cuda", generator=gen)
    bit = torch.randint(0, 8, (victims.numel(),), device="cuda", generator=gen).to(torch.uint8)
    data.view(-1)[pos] ^= (torch.ones_like(bit) << bit)
    rows.append(row("device_clean", *dev_flows, True))
    assert rows[-1]["nbad"] == 0 and rows[-1]["nsalvaged"] == 0 and rows[-1]["nitems"] == n, "the damage was not undone"

    # a page-locked host buffer of 1 and of 16 clean wbufs, the nkey of image 400 of the last wbuf zeroed
    for nwb in (1, 16):
        size, cap = nwb * wbuf, nwb * 1007
        p = lib.crc32c_host_alloc(size)
        assert p, "crc32c_host_alloc"
        host = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), (size,))
        host[:] = data.view(-1)[:size].cpu().numpy()
        host[(nwb - 1) * wbuf + 400 * 4165 + 41] = 0
        a = [np.empty(cap, np.uint64), np.empty(cap, np.uint8), np.empty(cap, np.uint64), np.empty(2 * cap, np.uint64),
             np.empty(2 * cap, np.uint32), np.empty(2 * cap, np.uint8)]
        rows.append(row(f"host_{nwb}", *flows(p, size, cap, 0, None, [x.ctypes.data for x in a]), False))
        assert rows[-1]["nsalvaged"] == 1007 - 401 and rows[-1]["nitems"] == cap - 1, rows[-1]
        lib.crc32c_host_free(p)

    lines.append(json.dumps({"summary": True, "pages": args.pages, "repeats": args.repeats,
                             "median_ms": {r["case"]: r["median_ms"] for r in rows},
                             "slower_rows": [r["case"] for r in rows if r["slower"]]}))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
