#!/usr/bin/env python3
"""crc32c_copy_items against the cheapest check-plus-copy the other calls
offer, on device-resident config-5 pages (bench.workload_config5: 1007 packed
4165-B images per 4 MiB wbuf, 1 % of them damaged).

    python tools/bench_copy_items.py [--pages 300] [--repeats 20] [--warmup 3] \
        [--out profiles/copy_items.jsonl]

For each keep share (25, 50 and 100 % of the images, every 4th, every 2nd and
every one, rescued into densely packed 4 MiB wbufs) one JSON line:

    copy_ms           median of `repeats` event-timed crc32c_copy_items calls
    verify_memcpy_ms  median of the same number of crc32c_verify_items calls
                      over the same images, each followed on the stream by one
                      device-to-device copy of the same byte count (torch's
                      copy of contiguous bytes, which issues hipMemcpyAsync; a
                      copy of no particular images: the least a separate copy
                      can cost)
    peak_fraction     (read + written rescued bytes) / copy time over 8 TB/s

one line for a single 1 MiB image (it stays on one 32-lane group), next to
crc32c_verify_items of the same image; and one line for the host route: both
buffers page-locked, one wbuf's images per call (host clock around the
synchronous call), next to the one-core loop memcpy + crc32c() over the same
images (tools/copy_host_loop.c, built with gcc into a temporary directory).
Every line holds all its samples.

--dst-align same gives the store-form A/B of DESIGN.md section 3.7: every
destination at its source's address mod 16, so that every 16-B store is
aligned.  --cases picks the lines; MCRC_LIB another build of the library.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8e12  # HBM bytes/s


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pages", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "copy_items.jsonl"))
    ap.add_argument("--cases", default="device,host,long", help="which lines to measure (comma-separated)")
    ap.add_argument("--dst-align", choices=["packed", "same"], default="packed",
                    help="device lines: destinations packed back to back (any alignment against the source), or "
                         "each at its source's address mod 16 in a 4176-B slot -- every 16-B store aligned: the "
                         "most a store form that realigns in registers could gain")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench
    from memcached_amd import _lib
    lib = _lib.lib
    cases = set(args.cases.split(","))
    if cases == {"long"}:
        args.pages = 1
    (base, nbytes, wbuf, _offs_p, n, _ok_p), _ok, _victims, _span_bytes, _meta = \
        bench.workload_config5(argparse.Namespace(pages=args.pages), 0, 1)
    offs = bench._KEEP[-1]
    per_wbuf, nt = 1007, 4165
    data = bench._KEEP[-2]
    st = torch.cuda.current_stream().cuda_stream
    nbad = ctypes.c_uint64(0)
    dev = _lib.CRC32C_DEVICE
    lines = []

    def timed(fn):
        ms = []
        for rep in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                ms.append(round(e0.elapsed_time(e1), 4))
        return ms

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for share in (25, 50, 100) if "device" in cases else ():
        soffs = offs[::100 // share].contiguous()
        k = soffs.numel()
        idx = torch.arange(k, device="cuda", dtype=torch.int64)
        if args.dst_align == "same":
            doffs = (idx * 4176 + soffs % 16).contiguous()
            dst = torch.empty(k * 4176 + 16, dtype=torch.uint8, device="cuda")
        else:
            doffs = ((idx // per_wbuf) * wbuf + (idx % per_wbuf) * nt).contiguous()
            dst = torch.empty(-(-k // per_wbuf) * wbuf, dtype=torch.uint8, device="cuda")
        ok = torch.empty(k, dtype=torch.uint8, device="cuda")
        moved = k * nt

        def copy():
            _lib.check(lib.crc32c_copy_items(base, nbytes, wbuf, soffs.data_ptr(), dst.data_ptr(), dst.numel(),
                                             doffs.data_ptr(), k, ok.data_ptr(), ctypes.byref(nbad), dev, st))

        def verify_memcpy():
            _lib.check(lib.crc32c_verify_items(base, nbytes, wbuf, soffs.data_ptr(), k, ok.data_ptr(),
                                               ctypes.byref(nbad), dev, st))
            dst[:moved].copy_(data[:moved], non_blocking=True)  # (contiguous bytes: torch issues hipMemcpyAsync D2D)

        c_ms = timed(copy)
        c_bad = int(nbad.value)
        # (a flipped header bit leaves a few images malformed, ok 0, or sane with
        # another length, which then overlap their neighbours in dst: counted, not compared)
        assert int((ok != 1).sum()) == c_bad
        v_ms = timed(verify_memcpy)
        assert int(nbad.value) == c_bad  # the same images fail either way
        med_c, med_v = statistics.median(c_ms), statistics.median(v_ms)
        emit({"case": "device", "dst_align": args.dst_align, "lib": os.path.basename(_lib.LIB_PATH), "pages": args.pages, "keep_percent": share, "images": k, "bytes_moved": moved,
              "nbad": c_bad, "copy_ms": med_c, "verify_memcpy_ms": med_v,
              "copy_over_verify_memcpy": round(med_c / med_v, 4),
              "peak_fraction": round(2 * moved / (med_c * 1e-3) / PEAK, 4),
              "copy_ms_samples": c_ms, "verify_memcpy_ms_samples": v_ms})
        del dst, ok, soffs, doffs

    if "long" in cases:
        # one 1 MiB image: it stays on its one 32-lane group (256 blocks in sequence)
        from memcached_amd import crc32c as mc
        from memcached_amd import layout
        img = layout.make_item(b"long01", bytes(range(256)) * 4095 + bytes(191), cas=1)
        assert len(img) == 1 << 20
        one = torch.zeros((1 << 20) + 64, dtype=torch.uint8, device="cuda")
        one[13:13 + len(img)] = torch.frombuffer(bytes(img), dtype=torch.uint8).cuda()
        so = torch.tensor([13], dtype=torch.int64, device="cuda")
        do = torch.tensor([6], dtype=torch.int64, device="cuda")
        _k, bad = mc.stamp_items(one, so)
        assert bad == 0
        dst1 = torch.empty((1 << 20) + 64, dtype=torch.uint8, device="cuda")
        ok1 = torch.empty(1, dtype=torch.uint8, device="cuda")

        def copy_long():
            _lib.check(lib.crc32c_copy_items(one.data_ptr(), one.numel(), 0, so.data_ptr(), dst1.data_ptr(),
                                             dst1.numel(), do.data_ptr(), 1, ok1.data_ptr(), ctypes.byref(nbad), dev, st))

        def verify_long():
            _lib.check(lib.crc32c_verify_items(one.data_ptr(), one.numel(), 0, so.data_ptr(), 1, ok1.data_ptr(),
                                               ctypes.byref(nbad), dev, st))

        c_ms = timed(copy_long)
        assert int(ok1[0]) == 1 and bool((dst1[6:6 + (1 << 20)] == one[13:13 + (1 << 20)]).all())
        v_ms = timed(verify_long)
        emit({"case": "one_image_1MiB", "bytes_moved": 1 << 20, "copy_ms": statistics.median(c_ms),
              "verify_items_ms": statistics.median(v_ms), "copy_ms_samples": c_ms, "verify_items_ms_samples": v_ms})

    if "host" not in cases:
        return finish(args, lines)
    # the host route: one wbuf's images per call, both buffers page-locked
    src_p, dst_p = lib.crc32c_host_alloc(wbuf), lib.crc32c_host_alloc(wbuf)
    assert src_p and dst_p
    src = np.ctypeslib.as_array((ctypes.c_uint8 * wbuf).from_address(src_p))
    src[:] = data[:wbuf].cpu().numpy()  # the pages' first wbuf
    h_offs = np.arange(per_wbuf, dtype=np.uint64) * nt
    h_ok = np.empty(per_wbuf, np.uint8)

    def host_copy():
        _lib.check(lib.crc32c_copy_items(src_p, wbuf, wbuf, h_offs.ctypes.data, dst_p, wbuf, h_offs.ctypes.data,
                                         per_wbuf, h_ok.ctypes.data, ctypes.byref(nbad), 0, None))

    us = []
    for rep in range(args.warmup + args.repeats):
        t0 = time.perf_counter()
        host_copy()
        t1 = time.perf_counter()
        if rep >= args.warmup:
            us.append(round((t1 - t0) * 1e6, 2))
    assert int((h_ok != 1).sum()) == nbad.value
    loop_us = None
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "copy_host_loop")
        libdir = os.path.dirname(_lib.LIB_PATH)
        subprocess.run(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tools", "copy_host_loop.c"), "-L", libdir, "-lmcrc32c",
                        f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
        r = subprocess.run([exe, str(wbuf), str(nt), str(per_wbuf), str(args.repeats)], capture_output=True,
                           text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        if r.returncode == 0:
            loop_us = float(r.stdout.strip())
    emit({"case": "host_both_pinned_one_wbuf", "images": per_wbuf, "bytes_moved": per_wbuf * nt, "nbad": int(nbad.value),
          "copy_us": statistics.median(us), "host_memcpy_crc32c_loop_us": loop_us, "copy_us_samples": us})
    lib.crc32c_host_free(src_p)
    lib.crc32c_host_free(dst_p)
    return finish(args, lines)


def finish(args, lines):
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
