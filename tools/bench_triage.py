#!/usr/bin/env python3
"""crc32c_triage_pages beside crc32c_recover_pages, and crc32c_recover_pages of
this build against another build's (the parent commit's) on the same pages.

    python tools/bench_triage.py [--pages 300] [--repeats 10] [--ab OLD.so --rounds 4]
                                 [--out profiles/triage_ab.jsonl]

In one process (as tools/bench_recover.py: the two calls alternate sample by
sample, medians of --repeats after --warmup, device events):
    device_damaged   device-resident config-5 pages (bench.workload_config5: 1007
                     packed 4165-B images per 4 MiB wbuf, one flipped bit in 1 %
                     of the images)
    device_clean     the same pages with the damage undone
Both calls' counts are compared on every row: with the suspects taken out they
are the same.  The triage adds no pass over the page's bytes, so it should cost
what recover costs plus the difference of its pick and merge.

With --ab OLD.so, crc32c_recover_pages alone is then measured in fresh
processes that alternate between OLD.so and this build's library (MCRC_LIB, as
profiles/repair_headline_ab.jsonl was made), --rounds of each: the feature must
leave it inside the spread of the old build's own samples.  Every sample is in
a raw JSON line, the last line is the summary.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(args, with_triage):
    """The rows of one process: a list of dicts."""
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from memcached_amd import _lib
    (base, nbytes, wbuf, _offs_p, n, _ok_p), _ok, _victims, _sb, _meta = \
        bench.workload_config5(argparse.Namespace(pages=args.pages), 0, 1)
    data, offs = bench._KEEP[-2], bench._KEEP[-1]
    lib = _lib.lib
    st = torch.cuda.current_stream().cuda_stream
    u64 = ctypes.c_uint64
    cap = 2 * n
    out = [torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda"),
           torch.empty(cap, dtype=torch.uint8, device="cuda")]
    ptrs = [x.data_ptr() for x in out]
    cr = [u64(0) for _ in range(5)]  # nitems, nbad, nsalvaged, scanned, ncand
    ct = [u64(0) for _ in range(6)]  # nitems, nbad, nsalvaged, nsuspect, scanned, ncand

    def recover():
        _lib.check(lib.crc32c_recover_pages(base, nbytes, wbuf, *ptrs, cap, *map(ctypes.byref, cr), _lib.CRC32C_DEVICE,
                                            st))

    def triage():
        _lib.check(lib.crc32c_triage_pages(base, nbytes, wbuf, *ptrs, cap, *map(ctypes.byref, ct), _lib.CRC32C_DEVICE,
                                           st))

    calls = (("recover", recover), ("triage", triage)) if with_triage else (("recover", recover),)

    def row(name):
        ms = {k: [] for k, _ in calls}
        for rep in range(args.warmup + args.repeats):
            for which, fn in calls:
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if rep >= args.warmup:
                    ms[which].append(round(e0.elapsed_time(e1), 4))
        r = [c.value for c in cr]
        rec = {"case": name, "ms": ms, "median_ms": {k: round(statistics.median(v), 4) for k, v in ms.items()},
               "nitems": r[0], "nbad": r[1], "nsalvaged": r[2], "scanned": r[3], "ncand": r[4]}
        if with_triage:
            t = [c.value for c in ct]
            assert (t[0] - t[3], t[1], t[2], t[4], t[5]) == tuple(r), (t, r)
            spread = round(max(ms["recover"]) - min(ms["recover"]), 4)
            rec.update(nsuspect=t[3], recover_spread_ms=spread,
                       triage_minus_recover=round(rec["median_ms"]["triage"] - rec["median_ms"]["recover"], 4))
        return rec

    rows = [row("device_damaged")]
    # the damage undone (bench.workload_config5's generator replayed, as tools/bench_recover.py does)
    gen = torch.Generator(device="cuda").manual_seed(3)
    victims = torch.randperm(n, device="cuda", generator=gen)[: n // 100]
    pos = offs[victims] + 32 + torch.randint(0, 4165 - 32, (victims.numel(),), device="cuda", generator=gen)
    bit = torch.randint(0, 8, (victims.numel(),), device="cuda", generator=gen).to(torch.uint8)
    data.view(-1)[pos] ^= (torch.ones_like(bit) << bit)
    rows.append(row("device_clean"))
    assert rows[-1]["nbad"] == 0 and rows[-1]["nsalvaged"] == 0 and rows[-1]["nitems"] == n, "the damage was not undone"
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pages", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ab", metavar="OLD.so", help="another build of the library: recover alone, in alternating fresh "
                    "processes")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triage_ab.jsonl"))
    args = ap.parse_args()

    if args.child:  # one fresh process of the A/B: recover alone, with the library MCRC_LIB names
        for rec in measure(args, False):
            print(json.dumps(rec), flush=True)
        return 0

    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    # the A/B first, each sample in a process of its own (this one has not touched the GPU yet)
    ab = {}
    if args.ab:
        new = os.path.join(ROOT, "memcached_amd", "libmcrc32c.so")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--pages", str(args.pages), "--repeats",
               str(args.repeats), "--warmup", str(args.warmup)]
        for rnd in range(1, args.rounds + 1):
            for name, path in (("parent", os.path.abspath(args.ab)), ("new", new)):
                r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, MCRC_LIB=path),
                                   timeout=600)
                if r.returncode != 0:
                    sys.stderr.write(r.stdout + r.stderr)
                    return 1
                for line in r.stdout.splitlines():
                    if line.startswith("{"):
                        rec = json.loads(line)
                        ab.setdefault(rec["case"], {}).setdefault(name, []).append(rec["median_ms"]["recover"])
                        emit({"ab": True, "round": rnd, "lib": name, **rec})
    rows = measure(args, True)
    for rec in rows:
        emit(rec)
    summary = {"summary": True, "pages": args.pages, "repeats": args.repeats,
               "median_ms": {r["case"]: r["median_ms"] for r in rows},
               "triage_minus_recover_ms": {r["case"]: r["triage_minus_recover"] for r in rows},
               "recover_spread_ms": {r["case"]: r["recover_spread_ms"] for r in rows},
               "nsuspect": {r["case"]: r["nsuspect"] for r in rows}}
    if ab:
        summary["recover_ab"] = {}
        for case, libs in ab.items():
            lo, hi = min(libs["parent"]), max(libs["parent"])
            med = round(statistics.median(libs["new"]), 4)
            summary["recover_ab"][case] = {"parent_ms": libs["parent"], "new_ms": libs["new"],
                                           "parent_median_ms": round(statistics.median(libs["parent"]), 4),
                                           "new_median_ms": med, "inside_parent_spread": lo <= med <= hi or med < lo}
    emit(summary)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
