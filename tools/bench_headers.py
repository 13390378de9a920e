#!/usr/bin/env python3
"""crc32c_repair_headers beside crc32c_recover_pages, in one process: the
read-back of device-resident config-5 pages with the bench's damage
(bench.workload_config5: 1007 packed 4165-B images per 4 MiB wbuf, one flipped
bit in 1 % of the images) as crc32c_recover_pages alone, and
crc32c_repair_headers alone over the list that read-back gives it: every
kind == 0 entry and every wbuf's walk end that is not itself an entry
(include/crc32c_batch.h).  The flows alternate sample by sample; medians of
--repeats after --warmup; every sample is in a raw JSON line, the last line is
the summary.  Descriptions, not thresholds.

    python tools/bench_headers.py [--pages 300] [--repeats 10] [--out profiles/headers.jsonl]

The timed calls run with CRC32C_LOCATE_ONLY, so that every sample sees the same
damage.  One more call afterwards repairs in place and crc32c_verify_items goes
over the repaired headers.

Rows:
    device      recover alone; the header call alone on its list (device
                events); of that the variants kernel's counting pass
                (crc32c_last_kernel_ms); headers repaired out of headers listed
    clean_list  crc32c_repair_headers and crc32c_verify_items over the same
                list of intact images, as many as the damaged list held
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_list(offs, lens, kind, nbytes, wbuf):
    """The list from crc32c_recover_pages' three arrays (numpy, ascending)."""
    import numpy as np
    walked = kind != 4
    o, ln, k = offs[walked], lens[walked].astype(np.uint64), kind[walked]
    w = o // np.uint64(wbuf)
    last = np.flatnonzero(np.r_[w[1:] != w[:-1], True]) if o.size else np.zeros(0, np.int64)
    good = last[k[last] == 1]
    ends = o[good] + ln[good]
    empty = np.setdiff1d(np.arange(-(-nbytes // wbuf), dtype=np.uint64), w[last]) * np.uint64(wbuf)
    ends = np.concatenate([ends, empty])
    pe = np.minimum((ends // np.uint64(wbuf) + np.uint64(1)) * np.uint64(wbuf), np.uint64(nbytes))
    # (a good last entry may end at its wbuf's end: that end belongs to no wbuf's walk)
    inside = (ends // np.uint64(wbuf) == np.concatenate([w[good], empty // np.uint64(wbuf)]))
    ends = ends[inside & (pe - ends >= 48)]
    return np.unique(np.concatenate([offs[kind == 0], ends])).astype(np.uint64)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pages", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "headers.jsonl"))
    args = ap.parse_args()

    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench
    from memcached_amd import _lib
    from memcached_amd import crc32c as mc
    (base, nbytes, wbuf, _offs_p, n, _ok_p), _ok, _victims, _sb, _meta = \
        bench.workload_config5(argparse.Namespace(pages=args.pages), 0, 1)
    data = bench._KEEP[-2]
    lib = _lib.lib
    st = torch.cuda.current_stream().cuda_stream
    u64 = ctypes.c_uint64
    lines = []
    cap = 2 * n
    moffs = torch.empty(cap, dtype=torch.int64, device="cuda")
    mlens = torch.empty(cap, dtype=torch.int32, device="cuda")
    mkind = torch.empty(cap, dtype=torch.uint8, device="cuda")
    counts = [u64(0) for _ in range(5)]
    nrep, nbad = u64(0), u64(0)

    def recover():
        _lib.check(lib.crc32c_recover_pages(base, nbytes, wbuf, moffs.data_ptr(), mlens.data_ptr(), mkind.data_ptr(), cap,
                                            *map(ctypes.byref, counts), _lib.CRC32C_DEVICE, st))

    recover()
    torch.cuda.synchronize()
    k = counts[0].value
    todo_h = header_list(moffs[:k].cpu().numpy().view(np.uint64), mlens[:k].cpu().numpy().view(np.uint32),
                         mkind[:k].cpu().numpy(), nbytes, wbuf)
    todo = torch.from_numpy(todo_h.view(np.int64)).cuda()
    m = todo.numel()
    hok = torch.empty(m, dtype=torch.uint8, device="cuda")
    hbit = torch.empty(m, dtype=torch.int64, device="cuda")
    hlens = torch.empty(m, dtype=torch.int32, device="cuda")

    def headers(lst, flags=_lib.CRC32C_LOCATE_ONLY):
        _lib.check(lib.crc32c_repair_headers(base, nbytes, wbuf, lst.data_ptr(), lst.numel(), hok.data_ptr(),
                                             hbit.data_ptr(), hlens.data_ptr(), ctypes.byref(nrep), ctypes.byref(nbad),
                                             _lib.CRC32C_DEVICE | flags, st))

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return round(e0.elapsed_time(e1), 4)

    def med(v):
        return round(statistics.median(v), 4)

    ms = {"recover": [], "header_call": [], "variants_kernel": []}
    for rep in range(args.warmup + args.repeats):
        a, b = timed(recover), timed(lambda: headers(todo))
        c = round(float(lib.crc32c_last_kernel_ms()), 4)
        if rep >= args.warmup:
            for key, v in zip(ms, (a, b, c)):
                ms[key].append(v)
    located = nrep.value
    kinds = np.bincount(hok.cpu().numpy(), minlength=6).tolist()
    # once more, in place, and the verify over the repaired headers
    headers(todo, 0)
    torch.cuda.synchronize()
    fixed = todo[hok == _lib.CRC32C_ITEM_REPAIRED].contiguous()
    _vok, vbad = mc.verify_items(data, fixed, region_bytes=wbuf)
    rec = {"case": "device", "pages": args.pages, "ms": ms, "median_ms": {k: med(v) for k, v in ms.items()},
           "recover_spread_ms": round(max(ms["recover"]) - min(ms["recover"]), 4), "images": n,
           "walk_bad": counts[1].value, "listed": m, "located": located, "repaired": nrep.value,
           "ok_histogram": kinds, "verify_of_repaired": {"n": fixed.numel(), "nbad": vbad}}
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)
    assert vbad == 0 and fixed.numel() == nrep.value == located

    # a clean list of the same length: the header call against the verify
    recover()
    torch.cuda.synchronize()
    k = counts[0].value
    clean = moffs[:k][mkind[:k] == 1][:m].contiguous()
    vok = torch.empty(clean.numel(), dtype=torch.uint8, device="cuda")
    vb = u64(0)

    def verify():
        _lib.check(lib.crc32c_verify_items(base, nbytes, wbuf, clean.data_ptr(), clean.numel(), vok.data_ptr(),
                                           ctypes.byref(vb), _lib.CRC32C_DEVICE, st))

    cms = {"verify_items": [], "repair_headers": []}
    for rep in range(args.warmup + args.repeats):
        a, b = timed(verify), timed(lambda: headers(clean))
        if rep >= args.warmup:
            cms["verify_items"].append(a)
            cms["repair_headers"].append(b)
    assert vb.value == 0 and nrep.value == 0 and nbad.value == 0
    lines.append(json.dumps({"case": "clean_list", "n": clean.numel(), "ms": cms,
                             "median_ms": {k: med(v) for k, v in cms.items()}}))
    print(lines[-1], flush=True)

    lines.append(json.dumps({"summary": True, "pages": args.pages, "repeats": args.repeats,
                             "median_ms": rec["median_ms"], "repaired": rec["repaired"], "listed": m,
                             "clean_list_median_ms": {k: med(v) for k, v in cms.items()}}))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
