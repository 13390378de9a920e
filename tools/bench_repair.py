#!/usr/bin/env python3
"""crc32c_repair_items behind crc32c_recover_pages, in one process: the
read-back of device-resident config-5 pages with the bench's damage
(bench.workload_config5: 1007 packed 4165-B images per 4 MiB wbuf, one flipped
bit in 1 % of the images) as crc32c_recover_pages alone, and as
crc32c_recover_pages followed by crc32c_repair_items over the entries with
kind == 0 && lens != 0.  The two flows alternate sample by sample; medians of
--repeats after --warmup; every sample is in a raw JSON line, the last line is
the summary.

    python tools/bench_repair.py [--pages 300] [--repeats 10] [--out profiles/repair.jsonl]

The timed repairs run with CRC32C_LOCATE_ONLY, so that every sample sees the
same damage (the search is the same; only the one byte store per image is
missing).  One more call afterwards repairs in place and crc32c_verify_items
goes over the repaired list.

Rows:
    device        recover alone; recover + list + repair; the repair call alone
                  (device events), the search kernel alone
                  (crc32c_last_kernel_ms), images repaired out of images given
    clean_list    crc32c_repair_items and crc32c_verify_items over the same
                  list of intact images, as many as the damaged list held: what
                  a list with nothing to repair costs
    host_wbuf     one page-locked wbuf (crc32c_host_alloc) of the damaged pages:
                  crc32c_repair_items over its bad entries, on the host clock
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repair.jsonl"))
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
    rok = torch.empty(cap, dtype=torch.uint8, device="cuda")
    rbit = torch.empty(cap, dtype=torch.int64, device="cuda")
    counts = [u64(0) for _ in range(5)]
    nrep, nbad = u64(0), u64(0)
    state = {}

    def recover():
        _lib.check(lib.crc32c_recover_pages(base, nbytes, wbuf, moffs.data_ptr(), mlens.data_ptr(), mkind.data_ptr(), cap,
                                            *map(ctypes.byref, counts), _lib.CRC32C_DEVICE, st))

    def bad_list():
        k = counts[0].value
        return moffs[:k][(mkind[:k] == 0) & (mlens[:k] != 0)].contiguous()

    def repair(todo, flags=_lib.CRC32C_LOCATE_ONLY):
        _lib.check(lib.crc32c_repair_items(base, nbytes, wbuf, todo.data_ptr(), todo.numel(), 0, rok.data_ptr(),
                                           rbit.data_ptr(), ctypes.byref(nrep), ctypes.byref(nbad),
                                           _lib.CRC32C_DEVICE | flags, st))

    def both():
        recover()
        state["todo"] = bad_list()
        repair(state["todo"])

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

    p = lib.crc32c_host_alloc(wbuf)
    assert p, "crc32c_host_alloc"
    host = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), (wbuf,))
    host[:] = data.view(-1)[:wbuf].cpu().numpy()

    ms = {"recover": [], "recover_repair": [], "repair_call": [], "search_kernel": []}
    for rep in range(args.warmup + args.repeats):
        a, b = timed(recover), timed(both)
        c = timed(lambda: repair(state["todo"]))
        k = round(float(lib.crc32c_last_kernel_ms()), 4)
        if rep >= args.warmup:
            for key, v in zip(ms, (a, b, c, k)):
                ms[key].append(v)
    given, located = state["todo"].numel(), nrep.value
    # once more, in place, and the verify over the repaired list
    recover()
    todo = bad_list()
    repair(todo, 0)
    torch.cuda.synchronize()
    fixed = todo[rok[:todo.numel()] == _lib.CRC32C_ITEM_REPAIRED].contiguous()
    vok, vbad = mc.verify_items(data, fixed, region_bytes=wbuf)
    rec = {"case": "device", "pages": args.pages, "ms": ms, "median_ms": {k: med(v) for k, v in ms.items()},
           "recover_spread_ms": round(max(ms["recover"]) - min(ms["recover"]), 4), "images": n,
           "walk_bad": counts[1].value, "given": given, "located": located, "repaired": nrep.value,
           "not_repaired": nbad.value, "verify_of_repaired": {"n": fixed.numel(), "nbad": vbad}}
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)
    assert vbad == 0 and fixed.numel() == nrep.value == located

    # a clean list of the same length: the repair against the verify
    recover()
    k = counts[0].value
    clean = moffs[:k][mkind[:k] == 1][:given].contiguous()
    vok = torch.empty(clean.numel(), dtype=torch.uint8, device="cuda")
    vb = u64(0)

    def verify():
        _lib.check(lib.crc32c_verify_items(base, nbytes, wbuf, clean.data_ptr(), clean.numel(), vok.data_ptr(),
                                           ctypes.byref(vb), _lib.CRC32C_DEVICE, st))

    cms = {"verify_items": [], "repair_items": []}
    for rep in range(args.warmup + args.repeats):
        a, b = timed(verify), timed(lambda: repair(clean))
        if rep >= args.warmup:
            cms["verify_items"].append(a)
            cms["repair_items"].append(b)
    assert vb.value == 0 and nrep.value == 0 and nbad.value == 0
    lines.append(json.dumps({"case": "clean_list", "n": clean.numel(), "ms": cms,
                             "median_ms": {k: med(v) for k, v in cms.items()}}))
    print(lines[-1], flush=True)

    # one page-locked host wbuf of the damaged pages (copied before the repair in place)
    offs_h, lens_h, kind_h, _info = mc.recover_pages(host, wbuf)
    todo_h = np.ascontiguousarray(offs_h[(kind_h == 0) & (lens_h != 0)])
    hms = []
    for rep in range(args.warmup + args.repeats):
        t0 = time.perf_counter()
        okh, bith, info = mc.repair_items(host, todo_h, region_bytes=wbuf, locate_only=True)
        if rep >= args.warmup:
            hms.append(round((time.perf_counter() - t0) * 1e3, 4))
    lines.append(json.dumps({"case": "host_wbuf", "given": int(todo_h.size), **info, "ms": hms, "median_ms": med(hms)}))
    print(lines[-1], flush=True)
    lib.crc32c_host_free(p)

    lines.append(json.dumps({"summary": True, "pages": args.pages, "repeats": args.repeats,
                             "median_ms": rec["median_ms"], "repaired": rec["repaired"], "given": given,
                             "clean_list_median_ms": {k: med(v) for k, v in cms.items()},
                             "repair_costs_more_than_recover": rec["median_ms"]["repair_call"] >
                             rec["median_ms"]["recover"]}))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
