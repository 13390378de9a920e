"""The op table of tests/interleave_cases.py, checked without a GPU: every
expectation is consistent in itself (counts match arrays, sentinels in place,
the error ops expect what include/crc32c_batch.h states), every op meets the
size conditions of the route it names (span_route through the host_route_check
program, item_route restated), the table reaches every exported batch entry
point, and every order puts a succeeding call of another entry point behind
each error."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import interleave_cases as ic

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OPS = ic.table()
IDS = [op.name for op in OPS]


def _body(a):
    """An expected output array without its sentinel, which must be there."""
    assert a[-1] == ic.SENT[a.itemsize]
    return a[:-1]


def _written(a):
    """The entries of an expected array the call writes: a prefix."""
    body = _body(a)
    k = int((body != ic.SENT[a.itemsize]).sum())
    assert (body[k:] == ic.SENT[a.itemsize]).all()
    return body[:k]


@pytest.mark.parametrize("op", OPS, ids=IDS)
def test_expectation_is_self_consistent(op):
    w, i = op.want, op.inputs
    for v in list(w.values()) + list(i.values()):
        if isinstance(v, np.ndarray):
            assert not v.flags.writeable
    if op.kind == "spans":
        assert _body(w["out"]).size == i["n"]
        if op.error:  # CRC32C_ERANGE: the span outside the buffer is not read and its entry is 0
            bad = op.extra["bad"]
            assert w["rc"] == ic.ERANGE and _body(w["out"])[bad] == 0
            assert int(i["offsets"][bad]) + int(i["lens"][bad]) > i["buf"].size
            inside = i["offsets"].astype(np.int64) + i["lens"] <= i["buf"].size
            assert (~inside).sum() == 1 and np.count_nonzero(_body(w["out"])[inside]) > 0.99 * (i["n"] - 1)
    elif op.kind == "chains":
        assert _body(w["iov_out"]).size == i["n"] and _body(w["out"]).size == i["nchains"] == i["first"].size - 1
        empty = np.diff(i["first"].astype(np.int64)) == 0
        assert (_body(w["out"])[empty] == 0).all()
    elif op.kind == "items":
        ok = _body(w["ok"])
        assert ok.size == i["offsets"].size and w["nbad"] == int((ok == 0).sum()) and 0 < w["nbad"] < ok.size
        assert set(ok.tolist()) <= ({0, 1} if i["flags"] == 0 else {0, 1, 2})
        if op.entry == "crc32c_stamp_items":
            changed = np.flatnonzero(w["buf"] != i["buf"])
            assert 0 < changed.size <= 4 * int((ok == 1).sum())
            assert set((changed[:, None] - i["offsets"][ok == 1].astype(np.int64)).ravel().tolist()) >= {28, 29, 30, 31}
    elif op.kind == "pages":
        offs, ok = _written(w["offsets"]), _body(w["ok"])[:_written(w["offsets"]).size]
        assert offs.size == min(i["cap"], w["nitems"]) and (np.diff(offs.astype(np.int64)) > 0).all()
        assert (ok != ic.SENT[1]).all() and (_body(w["ok"])[offs.size:] == ic.SENT[1]).all()
        assert w["nbad"] >= int((ok == 0).sum()) > 0  # (nbad covers the items behind cap too)
        if i["cap"] >= w["nitems"]:
            assert w["nbad"] == int((ok == 0).sum())
    elif op.kind == "salvage":
        found = _written(w["offsets"])
        if w["rc"] == ic.OK:
            assert w["nfound"] == found.size <= w["ncand"] <= w["scanned"] and i["cap"] > found.size
            assert (np.diff(found.astype(np.int64)) > 0).all()
        elif w["rc"] == ic.EWORK:  # nothing reported, *nfound = 0, *scanned and *ncand filled
            assert found.size == 0 and w["nfound"] == 0 and 0 < w["ncand"] <= w["scanned"] != ic.SENT64
        else:  # CRC32C_EINVAL: walked not strictly ascending, nothing is written
            assert w["rc"] == ic.EINVAL and found.size == 0
            assert w["nfound"] == w["scanned"] == w["ncand"] == ic.SENT64
            assert not (np.diff(i["walked"].astype(np.int64)) > 0).all()
    elif op.kind == "recover":
        offs, lens, kind = (_written(w[k]) for k in ("offsets", "lens", "kind"))
        assert offs.size == lens.size == kind.size == w["nitems"] < i["cap"]
        assert (np.diff(offs.astype(np.int64)) > 0).all()
        assert w["nbad"] == int((kind == 0).sum()) and w["nsalvaged"] == int((kind == 4).sum())
        assert set(kind.tolist()) <= {0, 1, 4} and (lens[kind != 0] >= 50).all()
        if op.error:  # CRC32C_EWORK: the walk's entries alone, *nsalvaged = 0, *scanned and *ncand filled
            assert w["rc"] == ic.EWORK and w["nsalvaged"] == 0 and w["nitems"] > 50 and 0 < w["ncand"] <= w["scanned"]
    elif op.kind == "repair":
        if op.error:  # CRC32C_EWORK: nothing is written into the buffer, *nrepaired = 0
            assert w["rc"] == ic.EWORK and w["nrepaired"] == 0 and np.array_equal(w["buf"], i["buf"])
            assert "ok" not in w and "bit" not in w and "nbad" not in w  # (unspecified)
        else:
            ok, bit = _body(w["ok"]), _body(w["bit"])
            assert w["nrepaired"] == int((ok == 5).sum()) > 300 and w["nbad"] == int((ok == 0).sum()) > 0
            assert ((bit != 2 ** 64 - 1) == (ok == 5)).all()
            flipped = int(np.unpackbits(w["buf"] ^ i["buf"]).sum())
            assert flipped == (0 if i["flags"] & ic.LOCATE_ONLY else w["nrepaired"])
    elif op.kind == "copy":
        ok = _body(w["ok"])
        assert w["nbad"] == int((ok != 1).sum()) > 0 and set(ok.tolist()) == {0, 1, 3}
        assert np.array_equal(w["src"], i["src"]) and (w["dst"] != 0xa5).sum() > 0.9 * w["dst"].size
        if op.error:  # CRC32C_ERANGE: a sane image that does not fit is not written, ok 0, counted
            assert w["rc"] == ic.ERANGE
            fits = ic.by_name("copy_device").want
            assert int((_body(fits["ok"]) != ok).sum()) == 1 and w["nbad"] == fits["nbad"] + 1
    elif op.kind == "queue":
        assert len(i["jobs"]) == 12 == w["nwaited"] and all(o.size <= 64 for o, _, _ in i["jobs"])
        assert w["out"].size == sum(o.size + 1 for o, _, _ in i["jobs"])
        assert max(int(ln.max()) for _, ln, _ in i["jobs"]) <= 256 << 10  # (coalescable spans)
    else:
        raise AssertionError(op.kind)


def test_error_ops_are_the_documented_codes():
    got = {op.name: op.want["rc"] for op in ic.error_ops()}
    assert got == {
        "spans_one_out_of_range": ic.ERANGE, "salvage_over_the_work_bound_device": ic.EWORK,
        "salvage_over_the_work_bound_host": ic.EWORK, "recover_over_the_work_bound": ic.EWORK,
        "salvage_list_not_ascending": ic.EINVAL, "repair_one_image_three_times": ic.EWORK,
        "copy_one_image_does_not_fit": ic.ERANGE}
    header = open(os.path.join(ROOT, "include", "crc32c_batch.h")).read()
    for name, value in (("CRC32C_EINVAL", ic.EINVAL), ("CRC32C_ERANGE", ic.ERANGE), ("CRC32C_EWORK", ic.EWORK)):
        assert re.search(rf"#define {name} \(({value})\)", header), name
    for name, value in (("CRC32C_DEVICE", ic.DEVICE), ("CRC32C_ASYNC", ic.ASYNC), ("CRC32C_KEEP_STAMPED", ic.KEEP_STAMPED),
                        ("CRC32C_LOCATE_ONLY", ic.LOCATE_ONLY)):
        assert re.search(rf"#define {name} 0x{value:x}u", header), name
    assert len(ic.success_ops()) >= 30


@pytest.fixture(scope="module")
def route_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("interleave") / "host_route_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "memcached_amd", "csrc"),
                    os.path.join(HERE, "integration", "host_route_check.cpp"), "-o", out], check=True)
    return out


def test_span_and_chain_ops_take_the_routes_they_name(route_exe):
    """span_route's own answer for every span and chain op that runs on the
    device (its base 16-B aligned, as device allocations are), at the
    small-batch limit the op runs with."""
    seen = set()
    for op in OPS:
        if op.kind not in ("spans", "chains") or op.where != "device":
            continue
        i = op.inputs
        args = [i["n"], i["length"], i["stride"], int(i["offsets"] is not None), int(i["lens"] is not None), 0,
                i.get("base_bytes", i["buf"].size), 8192 if op.small_max is None else op.small_max]
        r = subprocess.run([route_exe, "route"] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout.strip() == op.route, (op.name, r.stdout, r.stderr)
        if op.kind == "spans":
            seen.add(op.route)
    assert seen == {"k1", "small", "k5", "id_blocks", "id_spans", "id_final", "planned"}
    # the two sides of the small-batch limit, and the long spans past one 64 KiB segment
    assert ic.by_name("spans_small").inputs["n"] == 8192 and ic.by_name("spans_planned").inputs["n"] == 8193
    assert ic.by_name("spans_small").inputs["buf"].size <= 8 * ic.MiB
    assert int(ic.by_name("spans_long").inputs["lens"].max()) > 4 * ic.MiB


def test_item_and_page_ops_take_the_routes_they_name():
    routes = set()
    for op in OPS:
        if op.kind == "items":
            n, size = op.inputs["offsets"].size, op.inputs["buf"].size
            name = op.name.split("_")[2]
            assert n == int(name)
            want = {"64": "small", "4095": "planned", "4096": "k5"}[name]
            if op.where == "host" and op.entry == "crc32c_stamp_items" and name == "4096":
                want = "planned"  # (staged images are not stamped where they lie)
            assert op.route == want, op.name
            assert (size <= 8 * ic.MiB) == (name == "64") and (n >= 4096) == (name == "4096") and n <= 8192
            routes.add(op.route)
        elif op.kind == "pages":
            n, size = op.want["nitems"], op.inputs["buf"].size
            one = "_1_" in op.name
            assert (size <= 8 * ic.MiB and n <= 4096) == one and (n >= 4096) == (not one)
            assert op.inputs["cap"] in (n + 2, n - 3)
    assert routes == {"small", "planned", "k5"}


def test_table_covers_every_exported_batch_entry_point():
    """Every function of include/crc32c_batch.h that takes a batch: a
    crc32c_spans or the flags word."""
    header = open(os.path.join(ROOT, "include", "crc32c_batch.h")).read()
    decls = re.findall(r"^int (crc32c_\w+)\(([^;]*)\);", header, re.M)
    batch = {name for name, params in decls if "crc32c_spans" in params or "unsigned flags" in params}
    assert len(batch) == 12 and "crc32c_batch_submit" in batch and "crc32c_batch_wait" not in batch
    assert {op.entry for op in OPS} == batch
    assert {op.where for op in OPS} == {"device", "host", "pinned"}


def test_orders_separate_errors():
    orders = ic.orders()
    assert sorted(orders) == ["largest_first", "seed1", "seed2", "seed3", "seed4", "seed5", "seed6", "smallest_first"]
    names = sorted(IDS)
    for key, order in orders.items():
        assert sorted(op.name for op in order) == names, key
        for op, nxt in zip(order, order[1:] + [None]):
            if op.error:
                assert nxt is not None and not nxt.error and nxt.entry != op.entry, (key, op.name)
    assert len({tuple(op.name for op in order) for order in orders.values()}) == len(orders)
    first, last = orders["largest_first"], orders["smallest_first"]
    assert first[0].demand > 100 * first[-1].demand and last[-1].demand > 100 * last[0].demand
