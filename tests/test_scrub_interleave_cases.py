"""The scrub ops of tests/scrub_interleave_cases.py, checked without a GPU, and
the guard that goes with them: a fourth out-of-order table beside
tests/interleave_cases.py's, the header ops' and the triage ops'.

crc32c_scrub_pages takes its mode word and its stream in a struct, so the three
older guards (which go by a crc32c_spans, an identifier ending in `flags` or an
`unsigned` word in front of `void *stream` in the parameter list) do not see
it; this one goes by the struct: every `int crc32c_*` declaration of
include/crc32c_batch.h with a crc32c_scrub_opts parameter is an entry of this
table, and none of them is an entry of the other three."""
import os
import re

import numpy as np

from tests import header_interleave_cases as hic
from tests import interleave_cases as ic
from tests import scrub_interleave_cases as sic
from tests import triage_interleave_cases as tic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = sic.table()


def _scrub_entry_points():
    header = open(os.path.join(ROOT, "include", "crc32c_batch.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = re.findall(r"^int (crc32c_\w+)\(([^;{]*)\);", header, re.M)
    return {name for name, params in decls if re.search(r"\bcrc32c_scrub_opts\b", params)}


def test_the_table_covers_every_entry_point_with_scrub_opts():
    mine = {op.entry for op in OPS}
    assert mine == {sic.ENTRY} == _scrub_entry_points()
    others = [{op.entry for op in t} for t in (ic.table(), hic.table(), tic.table())]
    assert not any(mine & o for o in others)
    names = [{op.name for op in t} for t in (ic.table(), hic.table(), tic.table())]
    assert not any({op.name for op in OPS} & n for n in names)
    assert {op.where for op in OPS} == {"device", "host"}
    assert sum(op.error for op in OPS) == 2


def test_the_older_guards_do_not_see_the_declaration():
    header = open(os.path.join(ROOT, "include", "crc32c_batch.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    params, = re.findall(r"^int crc32c_scrub_pages\(([^;{]*)\);", header, re.M)
    assert not re.search(r"crc32c_spans|\w*flags\b|\bunsigned(\s+int)?\s+\w+\s*,\s*void\s*\*\s*stream", params)


def test_expectations_are_self_consistent():
    for op in OPS:
        w, i = op.want, op.inputs
        for v in list(w.values()) + list(i.values()):
            if isinstance(v, np.ndarray):
                assert not v.flags.writeable
        for (name, dtype), room in zip(sic.LISTS, [i["cap"]] * 3 + [i["flip_cap"]] * 3):
            assert w[name].size == room + 1 and w[name].dtype == dtype
        if w["rc"] == ic.EINVAL:
            assert np.array_equal(w["buf"], i["buf"]) and w["nitems"] == ic.SENT64
            continue
        k, kf = min(i["cap"], w["nitems"]), min(i["flip_cap"], w["nflips"])
        assert (w["offsets"][k:] == ic.SENT[8]).all() and (w["flip_by"][kf:] == ic.SENT[1]).all()
        assert (np.diff(w["offsets"][:k].astype(np.int64)) > 0).all()
        assert w["nflips"] == w["headers_repaired"] + w["items_repaired"]
        if op.error:
            assert w["rc"] == ic.EWORK and w["nflips"] == 0 and np.array_equal(w["buf"], i["buf"])
            continue
        assert set(w["flip_by"][:kf].tolist()) <= {1, 2} and w["rounds"] >= 1
        changed = int(np.unpackbits(w["buf"] ^ i["buf"]).sum())
        assert changed == (0 if i["mode"] & ic.LOCATE_ONLY else w["nflips"])
        assert w["complete"] == (0 if i["max_rounds"] == 1 else 1)


def test_orders_with_the_scrub_ops_separate_errors():
    ops = list(ic.orders()["seed2"])
    mixed = []
    for j, op in enumerate(ops):
        mixed.append(op)
        if j % 3 == 2:
            mixed.append(OPS[(j // 3) % len(OPS)])
    mixed = ic.separate_errors(mixed)
    assert sum(op.entry == sic.ENTRY for op in mixed) >= len(OPS)
    for op, nxt in zip(mixed, mixed[1:] + [None]):
        if op.error:
            assert nxt is not None and not nxt.error and nxt.entry != op.entry, op.name
