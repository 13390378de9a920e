#!/usr/bin/env python3
"""crc32c_scrub_pages beside the same flow written out over the existing entry
points, in one process, on the pages tools/bench_triage.py uses.

    python tools/bench_scrub.py [--pages 300] [--host-pages 30] [--repeats 10] [--warmup 2]
                                [--out profiles/scrub_ab.jsonl]

Rows (bench.workload_config5: 1007 packed 4165-B images per 4 MiB wbuf, one
flipped bit in 1 % of the images; clean: the damage undone):
    device_damaged, device_clean   device-resident pages
    host_damaged, host_clean       the first --host-pages pages in pageable host
                                   memory (the compaction case: every call of the
                                   written-out flow stages the page again)
One sample is one whole flow on a fresh copy of the page (restored outside the
timed region), wall clock around synchronous calls; the scrub and the
written-out flow alternate sample by sample, medians of --repeats after
--warmup.  The written-out flow is the contract's loop over
crc32c_triage_pages, crc32c_repair_headers and crc32c_repair_items through
ctypes, its two lists built on the host with numpy (for a device page the
triage's list comes to the host and the repair list goes back, as a caller's
would).  Both flows' final counts, flips and bytes are compared on every row.
The clean rows also time crc32c_triage_pages alone, the spread of its samples
being the margin tools/bench_triage.py uses.  written_out_list_building_ms is
the part of the written-out flow's time spent building its lists in numpy (a C
caller's loops take less).  Every sample is in a raw JSON
line, the last line is the summary.
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
u64 = ctypes.c_uint64


def header_list(offs, lens, kind, nbytes, W):
    """INTEGRATION.md 4f over numpy arrays: every kind-0 entry, and each
    piece's walk end when its last walked entry is not kind 0."""
    nw = -(-nbytes // W)
    walked = np.flatnonzero((kind == 0) | (kind == 1))
    ps = np.arange(nw, dtype=np.uint64) * np.uint64(W)
    pe = np.minimum(ps + np.uint64(W), np.uint64(nbytes))
    end, last = ps.copy(), np.ones(nw, np.uint8)
    if walked.size:
        piece = (offs[walked] // np.uint64(W)).astype(np.int64)
        tail = walked[np.flatnonzero(np.diff(piece, append=-1))]  # each piece's last walked entry
        w = (offs[tail] // np.uint64(W)).astype(np.int64)
        end[w] = offs[tail] + lens[tail].astype(np.uint64)
        last[w] = kind[tail]
    take = (last != 0) & (end >= ps) & (end <= pe) & (pe - np.minimum(end, pe) >= 48)
    return np.sort(np.concatenate((offs[kind == 0], end[take])))


def item_list(offs, lens, kind):
    """INTEGRATION.md 4g over numpy arrays."""
    keep = [offs[(kind == 0) & (lens != 0)]]
    sus = np.flatnonzero(kind == 6)
    if sus.size:
        proven = np.flatnonzero((kind == 1) | (kind == 4))
        at = np.searchsorted(proven, sus, side="right")
        nxt = np.full(sus.size, np.iinfo(np.uint64).max, np.uint64)
        nxt[at < proven.size] = offs[proven[at[at < proven.size]]]
        ends = offs[sus] + lens[sus].astype(np.uint64)
        kept, kept_end = [], 0
        for o, e in zip(offs[sus][ends <= nxt].tolist(), ends[ends <= nxt].tolist()):
            if o >= kept_end:
                kept.append(o)
                kept_end = e
        keep.append(np.array(kept, np.uint64))
    return np.sort(np.concatenate(keep))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pages", type=int, default=300)
    ap.add_argument("--host-pages", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scrub_ab.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from memcached_amd import _lib
    lib = _lib.lib
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
            todo_d, ok_d, bit_d, lens_d = new(cap, torch.int64), new(cap, torch.uint8), new(cap, torch.int64), new(
                cap, torch.int32)
            ptr, flag, stream = (lambda a: a.data_ptr()), _lib.CRC32C_DEVICE, st
            host = lambda a, k, d: a[:k].cpu().numpy().view(d)  # noqa: E731
        else:
            src = source.cpu().numpy()
            page = np.empty(nbytes, np.uint8)
            restore = lambda: np.copyto(page, src)  # noqa: E731
            arrays = [np.empty(cap, np.uint64), np.empty(cap, np.uint32), np.empty(cap, np.uint8),
                      np.empty(fcap, np.uint64), np.empty(fcap, np.uint64), np.empty(fcap, np.uint8)]
            todo_d, ok_d, bit_d, lens_d = (np.empty(cap, np.uint64), np.empty(cap, np.uint8), np.empty(cap, np.uint64),
                                           np.empty(cap, np.uint32))
            ptr, flag, stream = (lambda a: a.ctypes.data), 0, None
            host = lambda a, k, d: a[:k]  # noqa: E731
        base = ptr(page)
        counts = [u64(0) for _ in range(6)]
        ncalls, wo_calls, list_s, list_ms = [0], [0], [0.0], []

        def triage():
            ncalls[0] += 1
            _lib.check(lib.crc32c_triage_pages(base, nbytes, wbuf, *map(ptr, arrays[:3]), cap,
                                               *map(ctypes.byref, counts), flag, stream))
            k = counts[0].value
            assert k <= cap
            return host(arrays[0], k, np.uint64), host(arrays[1], k, np.uint32), host(arrays[2], k, np.uint8)

        def put(todo):
            if dev:
                todo_d[:todo.size].copy_(torch.from_numpy(todo.view(np.int64)))
            else:
                todo_d[:todo.size] = todo

        def written_out():
            """(flips as (offset, bit, by) lists, rounds)"""
            ncalls[0], list_s[0] = 0, 0.0
            log, rounds = [], 0
            T = triage()
            while True:
                nrep, nleft = u64(0), u64(0)
                t0 = time.perf_counter()
                todo = header_list(*T, nbytes, wbuf)
                list_s[0] += time.perf_counter() - t0
                by = 1
                if todo.size:
                    put(todo)
                    ncalls[0] += 1
                    _lib.check(lib.crc32c_repair_headers(base, nbytes, wbuf, ptr(todo_d), todo.size, ptr(ok_d),
                                                         ptr(bit_d), ptr(lens_d), ctypes.byref(nrep),
                                                         ctypes.byref(nleft), flag, stream))
                if nrep.value == 0:
                    t0 = time.perf_counter()
                    todo = item_list(*T)
                    list_s[0] += time.perf_counter() - t0
                    by = 2
                    if todo.size:
                        put(todo)
                        ncalls[0] += 1
                        _lib.check(lib.crc32c_repair_items(base, nbytes, wbuf, ptr(todo_d), todo.size, 0, ptr(ok_d),
                                                           ptr(bit_d), ctypes.byref(nrep), ctypes.byref(nleft), flag,
                                                           stream))
                    if nrep.value == 0:
                        wo_calls[0] = ncalls[0]
                        list_ms.append(round(list_s[0] * 1e3, 4))
                        return log, rounds
                hit = host(ok_d, todo.size, np.uint8) == 5
                log += [(o, b, by) for o, b in zip(todo[hit].tolist(), host(bit_d, todo.size, np.uint64)[hit].tolist())]
                rounds += 1
                T = triage()

        opts = _lib.ScrubOpts(flag, 0, 0, stream)
        out = _lib.ScrubOut(*map(ptr, arrays[:3]), cap, *map(ptr, arrays[3:]), fcap)

        def scrub():
            rc = lib.crc32c_scrub_pages(base, nbytes, wbuf, ctypes.byref(opts), ctypes.byref(out))
            _lib.check(rc)
            assert out.nflips <= fcap and out.nitems <= cap and out.complete == 1
            k = out.nflips
            return list(zip(host(arrays[3], k, np.uint64).tolist(), host(arrays[4], k, np.uint64).tolist(),
                            host(arrays[5], k, np.uint8).tolist())), out.rounds

        def alone():  # (the call by itself: its list stays where it is)
            _lib.check(lib.crc32c_triage_pages(base, nbytes, wbuf, *map(ptr, arrays[:3]), cap,
                                               *map(ctypes.byref, counts), flag, stream))
            return [], 0

        flows = [("scrub", scrub), ("written_out", written_out)] + ([("triage", alone)] if "clean" in name else [])
        ms, result, after = {k: [] for k, _ in flows}, {}, {}
        for rep in range(args.warmup + args.repeats):
            for which, fn in flows:
                restore()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                result[which] = fn()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    ms[which].append(round((time.perf_counter() - t0) * 1e3, 4))
                if rep == 0 and which != "triage":
                    after[which] = page.clone() if dev else page.copy()
        assert result["scrub"] == result["written_out"], "the two flows' logs differ"
        same = torch.equal(after["scrub"], after["written_out"]) if dev else bool(
            (after["scrub"] == after["written_out"]).all())
        assert same, "the two flows' pages differ"
        med = {k: round(statistics.median(v), 4) for k, v in ms.items()}
        rec = {"case": name, "bytes": nbytes, "ms": ms, "median_ms": med, "nitems": out.nitems, "nflips": out.nflips,
               "headers_repaired": out.headers_repaired, "items_repaired": out.items_repaired, "rounds": out.rounds,
               "calls_written_out": wo_calls[0], "written_out_list_building_ms": round(statistics.median(list_ms), 4),
               "written_out_over_scrub": round(med["written_out"] / med["scrub"], 3)}
        if "clean" in name:
            rec["triage_spread_ms"] = round(max(ms["triage"]) - min(ms["triage"]), 4)
            rec["scrub_minus_triage_ms"] = round(med["scrub"] - med["triage"], 4)
        emit(rec)
        return rec

    rows = [row("device_damaged", True, damaged, nbytes_all, n_all), row("device_clean", True, clean, nbytes_all, n_all)]
    hp = min(args.host_pages, args.pages)
    hb, hn = hp * 16 * wbuf, hp * 16 * 1007
    rows += [row("host_damaged", False, damaged.view(-1)[:hb], hb, hn), row("host_clean", False, clean.view(-1)[:hb], hb, hn)]
    emit({"summary": True, "pages": args.pages, "host_pages": hp, "repeats": args.repeats,
          "median_ms": {r["case"]: r["median_ms"] for r in rows},
          "written_out_over_scrub": {r["case"]: r["written_out_over_scrub"] for r in rows},
          "calls_written_out": {r["case"]: r["calls_written_out"] for r in rows},
          "rounds": {r["case"]: r["rounds"] for r in rows}, "nflips": {r["case"]: r["nflips"] for r in rows}})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
