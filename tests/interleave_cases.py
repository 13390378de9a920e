"""One table of library calls for the tests that run them out of order, after
errors and beside other kernels (tests/test_gpu_interleave.py).  No GPU and no
library call here: an op is a name, its inputs as read-only numpy arrays, a
run() that makes fresh copies, calls one entry point and returns everything the
call writes, and the expected values, which come from the oracle and the CPU
models under tests/ alone.  Inputs and expectations are built once per process.

Every output array an op hands to the library has one more entry than the call
may write, filled with a sentinel; run() returns the arrays whole and the
expected arrays end with the sentinel.  Side, the sentinels and the callers of
the page-recovery entry points are tests/raw_calls.py's."""
import ctypes
import functools
from dataclasses import dataclass, field

import numpy as np

from . import chain_cases as cc
from . import copy_cases
from . import copy_items_model
from . import oracle
from . import raw_calls
from . import recover_model
from . import repair_cases
from . import repair_model
from . import routes_cases as rc_
from . import salvage_cases as sc
from . import salvage_model as sm
from .raw_calls import (ASYNC, DEVICE, EINVAL, ERANGE, EWORK, KEEP_STAMPED, LOCATE_ONLY, OK,  # noqa: F401
                        RECOVER_COUNTS, SENT, SENT64, _capped, _lib, _ro, ended, ptr)

MiB = 1 << 20
# (the tables' arrays end with one sentinel word, not raw_calls.EXTRA)
Side = functools.partial(raw_calls.Side, pad=1)


def _u64(v=SENT64):
    return ctypes.c_uint64(v)


@dataclass(eq=False)
class Op:
    name: str
    entry: str            # the exported entry point it calls
    where: str            # "device", "host" or "pinned"
    inputs: dict          # read-only numpy arrays and plain numbers
    want: dict            # what run() must return: rc, arrays (ended), counts
    call: object          # call(op, side) -> dict
    route: str = ""       # the route its name promises (spans, chains: span_route; items: item_route)
    small_max: object = None  # crc32c_set_small_max for the route (chains); None: the default
    demand: int = 0       # about how much scratch the call needs, for the orders by size
    kind: str = ""
    extra: dict = field(default_factory=dict)

    def __post_init__(self):
        for v in list(self.inputs.values()) + list(self.want.values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)

    @property
    def error(self):
        return self.want["rc"] != OK

    def run(self, torch, stream=None, where=None):
        with Side(torch, stream, where or self.where) as side:
            return self.call(self, side)


def check(op, got, tag=""):
    """Everything a run returned against the op's expectation, exactly."""
    assert sorted(got) == sorted(op.want), (op.name, tag, sorted(got), sorted(op.want))
    for key, want in op.want.items():
        if isinstance(want, np.ndarray):
            np.testing.assert_array_equal(got[key], want, err_msg=f"{op.name} {tag}: {key}")
        else:
            assert got[key] == want, (op.name, tag, key, got[key], want)


# -- spans -----------------------------------------------------------------------

def spans_struct(side, op, buf, out):
    i = op.inputs
    offs, lens, cin = side.desc(i.get("offsets")), side.desc(i.get("lens")), side.desc(i.get("crc_in"))
    s = _lib().Spans(ptr(buf), i.get("base_bytes", i["buf"].size), ptr(offs), i.get("stride", 0), ptr(lens),
                     i.get("length", 0), ptr(cin), ptr(out), i["n"])
    s.keep = buf, offs, lens, cin, out  # (the struct holds bare addresses)
    return s


def _call_spans(op, side):
    buf = side.data(op.inputs["buf"])
    out = side.out(op.inputs["n"], np.uint32)
    s = spans_struct(side, op, buf, out)
    if op.entry == "crc32c_batch_multi":
        rc = _lib().lib.crc32c_batch_multi(ctypes.byref(s), 1)
    else:
        rc = _lib().lib.crc32c_batch(ctypes.byref(s), side.flags(), side.handle)
    return {"rc": rc, "out": side.host(out, np.uint32)}


def _spans_op(name, where, route, buf, n, *, offsets=None, stride=0, lens=None, length=0, crc_in=None, want=None,
              rc=OK, base_bytes=None, entry="crc32c_batch"):
    inputs = {"buf": buf, "n": n, "offsets": offsets, "stride": stride, "lens": lens, "length": length,
              "crc_in": crc_in}
    if base_bytes is not None:
        inputs["base_bytes"] = base_bytes
    if want is None:
        o = offsets if offsets is not None else np.arange(n, dtype=np.uint64) * np.uint64(stride)
        want = oracle.batch(buf, o, lens if lens is not None else np.full(n, length, np.uint64), crc_in)
    return Op(name, entry, where, inputs, {"rc": rc, "out": ended(want, np.uint32)}, _call_spans, route=route,
              demand=buf.size // 64 + 64 * n, kind="spans")


def _fixed_spans(length, seed):
    """8193 disjoint spans of one length by offsets, at 8193 starts that take
    every residue mod 128, with initial CRCs."""
    rng = np.random.default_rng(seed)
    n = 8193
    offs, size = cc._mixed_offsets(n, length)
    buf = _ro(rng.integers(0, 256, size, dtype=np.uint8))
    cin = _ro(rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32))
    return buf, _ro(offs), cin, n


def _span_ops():
    ops = []
    buf, offs, lens, want = rc_.short_spans()
    for n, route in ((8192, "small"), (8193, "planned")):
        ops.append(_spans_op(f"spans_{route}", "device", route, buf, n, offsets=_ro(offs[:n].copy()),
                             lens=_ro(lens[:n].copy()), want=want[:n]))
    ops.append(_spans_op("spans_small_host", "host", "small", buf, 8192, offsets=_ro(offs[:8192].copy()),
                         lens=_ro(lens[:8192].copy()), want=want[:8192]))
    ops.append(_spans_op("spans_multi_host", "host", "planned", buf, 8193, offsets=_ro(offs.copy()),
                         lens=_ro(lens.copy()), want=want, entry="crc32c_batch_multi"))
    # (500 B is k_spans' too: with kWholeMax = 512 the final-only route ends at 385 B, so 300 B stands for it)
    for length, route in ((4133, "k5"), (4090, "id_blocks"), (5000, "id_spans"), (500, "id_spans"), (300, "id_final")):
        b, o, cin, n = _fixed_spans(length, 7000 + length)
        ops.append(_spans_op(f"spans_{length}_{route}", "device", route, b, n, offsets=o, length=length, crc_in=cin))
    # 60 spans of up to 5 MiB, unaligned (several 64 KiB units each: split and combined)
    rng = np.random.default_rng(31)
    lens = rng.integers(0, 5 << 20, 60).astype(np.uint32)
    lens[:6] = [65536, 65537, 65535, 131072, 131073, (3 << 20) + 5]
    offs = np.concatenate([[7], 7 + np.cumsum(lens[:-1].astype(np.uint64) + 7)]).astype(np.uint64)
    buf = _ro(rng.integers(0, 256, int(offs[-1] + lens[-1] + 64), dtype=np.uint8))
    cin = _ro(rng.integers(0, 2 ** 32, lens.size, dtype=np.uint64).astype(np.uint32))
    ops.append(_spans_op("spans_long", "device", "planned", buf, 60, offsets=_ro(offs), lens=_ro(lens), crc_in=cin))
    # one span outside the buffer: not read, its entry 0, CRC32C_ERANGE, the rest exact
    rng = np.random.default_rng(77)
    buf = _ro(rng.integers(0, 256, 1 << 20, dtype=np.uint8))
    n, bad = 500, 77
    offs = rng.integers(0, buf.size - 5000, n).astype(np.uint64)
    lens = rng.integers(0, 5000, n).astype(np.uint32)
    offs[bad], lens[bad] = buf.size - 10, 11
    good = np.arange(n) != bad
    want = np.zeros(n, np.uint32)
    want[good] = oracle.batch(buf, offs[good], lens[good])
    ops.append(_spans_op("spans_one_out_of_range", "device", "small", buf, n, offsets=_ro(offs), lens=_ro(lens),
                         want=want, rc=ERANGE))
    ops[-1].extra["bad"] = bad
    # K1: 4099 items of 4 KiB (no multiple of the 32 per block step), with initial CRCs
    rng = np.random.default_rng(42)
    n = 4099
    buf = _ro(rng.integers(0, 256, n * 4096, dtype=np.uint8))
    cin = _ro(rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32))
    ops.append(_spans_op("k1_4099", "device", "k1", buf, n, stride=4096, length=4096, crc_in=cin))
    return ops


# -- chains ----------------------------------------------------------------------

def _call_chains(op, side):
    i = op.inputs
    buf = side.data(i["buf"])
    iov_out, out = side.out(i["n"], np.uint32), side.out(i["nchains"], np.uint32)
    s = spans_struct(side, op, buf, iov_out)
    first = side.desc(i["first"])
    rc = _lib().lib.crc32c_batch_chains(ctypes.byref(s), ptr(first), i["nchains"], ptr(out), side.flags(), side.handle)
    return {"rc": rc, "iov_out": side.host(iov_out, np.uint32), "out": side.host(out, np.uint32)}


def _chain_ops():
    ops = []
    for case in cc.route_cases() + cc.zero_cases():
        inputs = {"buf": _ro(case.buf), "n": case.n, "offsets": case.offsets, "stride": case.stride, "lens": case.lens,
                  "length": case.length, "first": _ro(case.first), "nchains": case.nchains}
        for a in (case.offsets, case.lens):
            if a is not None:
                _ro(a)
        want = {"rc": OK, "iov_out": ended(cc.expected_iovs(case), np.uint32), "out": ended(cc.expected(case), np.uint32)}
        ops.append(Op(f"chains_{case.name}", "crc32c_batch_chains", "device", inputs, want, _call_chains,
                      route=case.route, small_max=case.small_max, demand=case.buf.size // 64 + 64 * case.n,
                      kind="chains"))
    host = ops[0]
    ops.append(Op(host.name + "_host", host.entry, "host", host.inputs, host.want, _call_chains, route=host.route,
                  demand=host.demand, kind="chains"))
    return ops


# -- item images -----------------------------------------------------------------

def _call_items(op, side):
    i = op.inputs
    buf, offs = side.data(i["buf"]), side.desc(i["offsets"])
    n = i["offsets"].size
    ok, nbad = side.out(n, np.uint8), _u64()
    fn = getattr(_lib().lib, op.entry)
    rc = fn(ptr(buf), i["buf"].size, 0, ptr(offs), n, ptr(ok), ctypes.byref(nbad), side.flags() | i["flags"],
            side.handle)
    got = {"rc": rc, "ok": side.host(ok, np.uint8), "nbad": nbad.value}
    if "buf" in op.want:
        got["buf"] = side.host(buf, np.uint8)
    return got


def item_route(n, base_bytes, device, stamp):
    """host_route.h item_route with the default small-batch limit (k5_ok: a
    host stamp's staged images cannot be stamped where they lie)."""
    if n <= 8192 and base_bytes <= 8 * MiB:
        return "small"
    return "k5" if n >= 4096 and (device or not stamp) else "planned"


def _item_ops():
    ops = []
    for name in ("64", "4095", "4096"):
        buf, offs = rc_.items_case(name)
        for mode in ("verify", "stamp", "keep"):
            w_buf, w_ok, w_bad = rc_.items_want(name, mode)
            for where in ("device", "host"):
                want = {"rc": OK, "ok": ended(w_ok, np.uint8), "nbad": w_bad}
                if mode != "verify":
                    want["buf"] = _ro(w_buf)
                inputs = {"buf": buf, "offsets": _ro(offs), "flags": KEEP_STAMPED if mode == "keep" else 0}
                ops.append(Op(f"items_{mode}_{name}_{where}",
                              "crc32c_verify_items" if mode == "verify" else "crc32c_stamp_items", where, inputs, want,
                              _call_items, route=item_route(offs.size, buf.size, where == "device", mode != "verify"),
                              demand=(0 if where == "device" else buf.size) + 64 * offs.size, kind="items"))
    return ops


# -- pages -----------------------------------------------------------------------

def _call_pages(op, side):
    i = op.inputs
    buf = side.data(i["buf"])
    cap = i["cap"]
    offs, ok = side.out(cap, np.uint64), side.out(cap, np.uint8)
    nitems, nbad = _u64(), _u64()
    fn = getattr(_lib().lib, op.entry)
    rc = fn(ptr(buf), i["buf"].size, i["wbuf"], ptr(offs), ptr(ok), cap, ctypes.byref(nitems), ctypes.byref(nbad),
            side.flags() | i["flags"], side.handle)
    got = {"rc": rc, "offsets": side.host(offs, np.uint64), "ok": side.host(ok, np.uint8), "nitems": nitems.value,
           "nbad": nbad.value}
    if "buf" in op.want:
        got["buf"] = side.host(buf, np.uint8)
    return got


def _page_ops():
    ops = []
    for nwbufs in (1, 5):
        buf, walked = rc_.pages_case(nwbufs)
        v_ok, (s_buf, s_ok, s_bad), _ = rc_.pages_want(nwbufs)
        n = walked.size
        for cap_kind, cap in (("full", n + 2), ("short", n - 3)):
            for where in ("device", "host") if (nwbufs, cap_kind) == (1, "full") else ("device",):
                base = {"buf": buf, "wbuf": rc_.WBUF, "cap": cap}
                counts = {"rc": OK, "offsets": _capped(walked, cap, np.uint64), "nitems": n}
                ops.append(Op(f"pages_verify_{nwbufs}_{cap_kind}_{where}", "crc32c_verify_pages", where,
                              dict(base, flags=0), dict(counts, ok=_capped(v_ok, cap, np.uint8),
                                                        nbad=int((v_ok == 0).sum())),
                              _call_pages, demand=buf.size // 256 + 64 * n + (0 if where == "device" else buf.size),
                              kind="pages"))
                ops.append(Op(f"pages_keep_{nwbufs}_{cap_kind}_{where}", "crc32c_stamp_pages", where,
                              dict(base, flags=KEEP_STAMPED), dict(counts, ok=_capped(s_ok, cap, np.uint8), nbad=s_bad,
                                                                   buf=_ro(s_buf)),
                              _call_pages, demand=buf.size // 256 + 64 * n + (0 if where == "device" else buf.size),
                              kind="pages"))
    return ops


# -- salvage and recover ---------------------------------------------------------

def _stated(op, got, n=None):
    """The part of a raw caller's result that the op states: its "buf" is the
    call's "after", and behind CRC32C_EWORK only the word behind each array's n entries."""
    got = dict(got, buf=got["after"])
    got.update((key, int(got[key[:-4]][n])) for key in op.want if key.endswith("_end"))
    return {key: got[key] for key in op.want}


def _call_salvage(op, side):
    i = op.inputs
    return _stated(op, raw_calls.salvage_pages(side, i["buf"], i["wbuf"], i["walked"], i["walked_ok"], cap=i["cap"]))


def _salvage_op(name, where, buf, W, walked=None, wok=None, refused=False):
    if walked is None:
        walked, wok = sc.walk_lists(buf, W)
    inputs = {"buf": _ro(buf), "wbuf": W, "walked": _ro(walked), "walked_ok": _ro(wok)}
    if refused:  # nothing is written
        inputs["cap"] = 8
        want = {"rc": EINVAL, "offsets": _capped([], 8, np.uint64), "nfound": SENT64, "scanned": SENT64,
                "ncand": SENT64}
    else:
        found, scanned, ncand, work = sm.salvage_fast(buf, W, walked, wok)
        over = work > sm.WORK_MAX * (scanned + W)
        inputs["cap"] = len(found) + 3
        want = {"rc": EWORK if over else OK, "offsets": _capped([] if over else found, inputs["cap"], np.uint64),
                "nfound": 0 if over else len(found), "scanned": scanned, "ncand": ncand}
    return Op(name, "crc32c_salvage_pages", where, inputs, want, _call_salvage,
              demand=buf.size // 128 + (0 if where == "device" else buf.size), kind="salvage")


def _call_recover(op, side):
    i = op.inputs
    return _stated(op, raw_calls.listed_pages(op.entry, side, i["buf"], i["wbuf"], cap=i["cap"]))


def _recover_op(name, where, buf, W):
    m = recover_model.recover(buf, W)
    cap = m["nitems"] + 3
    want = {"rc": m["rc"], "offsets": _capped(m["offsets"], cap, np.uint64), "lens": _capped(m["lens"], cap, np.uint32),
            "kind": _capped(m["kind"], cap, np.uint8)}
    want.update((k, m[k]) for k in RECOVER_COUNTS)
    return Op(name, "crc32c_recover_pages", where, {"buf": _ro(buf), "wbuf": W, "cap": cap}, want, _call_recover,
              demand=buf.size // 64 + (0 if where == "device" else buf.size), kind="recover")


def _salvage_ops():
    ops = []
    cases = sc.small_cases()
    for name in ("data_only", "ranges_over_64", "config5_small"):
        buf, W, cfl = cases[name]
        assert cfl == 4
        for where in ("device", "host") if name == "ranges_over_64" else ("device",):
            ops.append(_salvage_op(f"salvage_{name}_{where}", where, buf, W))
            ops.append(_recover_op(f"recover_{name}_{where}", where, buf, W))
    buf, W = sc.work_bound_case()
    ops.append(_salvage_op("salvage_over_the_work_bound_device", "device", buf, W))
    ops.append(_salvage_op("salvage_over_the_work_bound_host", "host", buf, W))
    buf, W = recover_model.work_bound_behind_a_walk()
    ops.append(_recover_op("recover_over_the_work_bound", "device", buf, W))
    buf, W, _ = cases["hdr_nkey0"]
    walked, _ = sc.walk_lists(buf, W)
    assert walked.size >= 4
    ops.append(_salvage_op("salvage_list_not_ascending", "device", buf, W, walked[::-1].copy(),
                           np.ones(walked.size, np.uint8), refused=True))
    return ops


# -- repair ----------------------------------------------------------------------

def _call_repair(op, side):
    i = op.inputs
    got = raw_calls.repair_items(side, i["buf"], i["offsets"], max_span=i["max_span"],
                                 locate_only=bool(i["flags"] & LOCATE_ONLY))
    return _stated(op, got, i["offsets"].size)


def _repair_ops():
    ops = []
    buf, offs, _ = repair_cases.mixed(np.random.default_rng(5), 2000, 1000)
    _ro(buf), _ro(offs)
    for mode, flags in (("in_place", 0), ("locate_only", LOCATE_ONLY)):
        ok, bit, nrep, nbad, after = repair_model.repair(buf, offs, max_span=1000, locate_only=bool(flags))
        want = {"rc": OK, "ok": ended(ok, np.uint8), "bit": ended(bit, np.uint64), "nrepaired": nrep, "nbad": nbad,
                "buf": _ro(after)}
        for where in ("device", "host"):
            ops.append(Op(f"repair_{mode}_{where}", "crc32c_repair_items", where,
                          {"buf": buf, "offsets": offs, "max_span": 1000, "flags": flags}, want, _call_repair,
                          demand=64 * offs.size + (0 if where == "device" else buf.size), kind="repair"))
    # one damaged image of 100 000 B listed three times: its spans pass base_bytes
    rng = np.random.default_rng(6)
    nt = 100000
    img = sc.image_nt(rng, nt)
    buf, offs = repair_cases.place([sc.image_nt(rng, 300), img, sc.image_nt(rng, 120000), sc.image_nt(rng, 300)])
    repair_cases.flip(buf, int(offs[1]), 8 * 5000 + 2)
    assert 3 * (nt - 32) > buf.size > 2 * (nt - 32)
    three = _ro(np.array([offs[1]] * 3 + [offs[0]], np.uint64))
    want = {"rc": EWORK, "nrepaired": 0, "buf": _ro(buf), "ok_end": SENT[1], "bit_end": SENT[8]}
    ops.append(Op("repair_one_image_three_times", "crc32c_repair_items", "device",
                  {"buf": buf, "offsets": three, "max_span": 0, "flags": 0}, want, _call_repair, demand=buf.size,
                  kind="repair"))
    return ops


# -- copy ------------------------------------------------------------------------

def _call_copy(op, side):
    i = op.inputs
    src, dst = side.data(i["src"]), side.data(i["dst_init"])
    so, do = side.desc(i["src_offsets"]), side.desc(i["dst_offsets"])
    n = i["src_offsets"].size
    ok, nbad = side.out(n, np.uint8), _u64()
    rc = _lib().lib.crc32c_copy_items(ptr(src), i["src"].size, i["wbuf"], ptr(so), ptr(dst), i["dst_init"].size, ptr(do),
                                      n, ptr(ok), ctypes.byref(nbad), side.flags(), side.handle)
    return {"rc": rc, "ok": side.host(ok, np.uint8), "nbad": nbad.value, "dst": side.host(dst, np.uint8),
            "src": side.host(src, np.uint8)}


def _copy_op(name, where, dst_bytes):
    src, soffs, doffs, used, _, _ = copy_cases.mixed_case()
    dst_init = _ro(np.full(dst_bytes(used), 0xa5, np.uint8))
    w_dst, w_ok, w_bad, w_erange = copy_items_model.expected_copy(src, soffs, copy_cases.WBUF, dst_init, doffs)
    want = {"rc": ERANGE if w_erange else OK, "ok": ended(w_ok, np.uint8), "nbad": w_bad, "dst": _ro(w_dst), "src": src}
    inputs = {"src": src, "src_offsets": _ro(soffs), "dst_init": dst_init, "dst_offsets": _ro(doffs),
              "wbuf": copy_cases.WBUF}
    return Op(name, "crc32c_copy_items", where, inputs, want, _call_copy, demand=64 * soffs.size, kind="copy")


def _copy_ops():
    return [_copy_op("copy_device", "device", lambda used: used), _copy_op("copy_pinned", "pinned", lambda used: used),
            # dst ends one byte short of the last sane image
            _copy_op("copy_one_image_does_not_fit", "device", lambda used: used - 1)]


# -- the queue -------------------------------------------------------------------

def _call_queue(op, side):
    lib = _lib()
    buf = side.data(op.inputs["buf"])
    jobs, rcs = [], []
    for offs, lens, cin in op.inputs["jobs"]:
        out = np.full(offs.size + 1, SENT[4], np.uint32)
        s = lib.Spans(ptr(buf), buf.size, ptr(offs), 0, ptr(lens), 0, ptr(cin), ptr(out), offs.size)
        handle = ctypes.c_void_p()
        rcs.append(lib.lib.crc32c_batch_submit(ctypes.byref(s), 0, ctypes.byref(handle)))
        jobs.append((s, handle, out))
    for (_, handle, _), rc in zip(jobs, list(rcs)):
        if rc == OK:
            rcs.append(lib.lib.crc32c_batch_wait(handle))
    return {"rc": next((rc for rc in rcs if rc != OK), OK), "nwaited": len(rcs) - len(jobs),
            "out": np.concatenate([out for _, _, out in jobs])}


def _queue_op():
    """12 jobs of at most 64 spans of at most 4 KiB in one page-locked buffer:
    every one can share a launch."""
    rng = np.random.default_rng(12)
    buf = _ro(rng.integers(0, 256, 1 << 20, dtype=np.uint8))
    jobs, outs = [], []
    for j in range(12):
        n = 64 if j % 5 == 0 else int(rng.integers(1, 65))
        lens = _ro(rng.integers(0, 4097, n).astype(np.uint32))
        offs = _ro(rng.integers(0, buf.size - 4096, n).astype(np.uint64))
        cin = None if j % 3 == 0 else _ro(rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32))
        jobs.append((offs, lens, cin))
        outs.append(ended(oracle.batch(buf, offs, lens, cin), np.uint32))
    want = {"rc": OK, "nwaited": 12, "out": _ro(np.concatenate(outs))}
    return Op("queue_12_jobs", "crc32c_batch_submit", "pinned", {"buf": buf, "jobs": tuple(jobs)}, want, _call_queue,
              demand=64 * 12 * 64, kind="queue")


# -- the table -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def table():
    """Every op, in a fixed order."""
    ops = (_span_ops() + _chain_ops() + _item_ops() + _page_ops() + _salvage_ops() + _repair_ops() + _copy_ops() +
           [_queue_op()])
    assert len({op.name for op in ops}) == len(ops)
    return tuple(ops)


def by_name(name):
    return next(op for op in table() if op.name == name)


def error_ops():
    return [op for op in table() if op.error]


def success_ops():
    return [op for op in table() if not op.error]


def separate_errors(order):
    """The order with every error op followed by an op of another entry point
    that succeeds: where it is not, the nearest such op behind it is moved up
    (or, at the end, the nearest one in front of it is moved behind)."""
    order = list(order)
    i = 0
    while i < len(order):
        op = order[i]
        if op.error and (i + 1 == len(order) or order[i + 1].error or order[i + 1].entry == op.entry):
            fits = [k for k in range(len(order)) if k != i and not order[k].error and order[k].entry != op.entry
                    and not (k and order[k - 1].error and k - 1 != i)]
            k = min(fits, key=lambda k: (k < i, abs(k - i)))
            moved = order.pop(k)
            i -= k < i
            order.insert(i + 1, moved)
        i += 1
    return order


def orders():
    """name -> order: six seeded permutations of the table, and the ops from the
    largest scratch demand to the smallest and back."""
    ops = list(table())
    out = {}
    for seed in (1, 2, 3, 4, 5, 6):
        perm = np.random.default_rng(9000 + seed).permutation(len(ops))
        out[f"seed{seed}"] = separate_errors([ops[k] for k in perm])
    by_size = sorted(ops, key=lambda op: -op.demand)
    out["largest_first"] = separate_errors(by_size)
    out["smallest_first"] = separate_errors(by_size[::-1])
    return out
