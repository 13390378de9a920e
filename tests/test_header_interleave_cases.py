"""The header ops of tests/header_interleave_cases.py, checked without a GPU,
and the guard that goes with them: every function of include/crc32c_batch.h
that takes a batch -- a crc32c_spans or the flags word, however the word's type
is spelt -- is an entry of the out-of-order table of tests/interleave_cases.py
or of the header ops' table, which tests/test_gpu_interleave_headers.py runs
among the former's.

crc32c_repair_headers declares its flags word `unsigned int flags`:
tests/test_interleave_cases.py pins the declarations that say `unsigned flags`
at the twelve its own table holds.  This test counts both spellings, so a
further entry point cannot stay outside both tables by its spelling."""
import os
import re

import numpy as np

from tests import header_interleave_cases as hic
from tests import interleave_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = hic.table()


def test_the_two_tables_cover_every_batch_entry_point():
    header = open(os.path.join(ROOT, "include", "crc32c_batch.h")).read()
    decls = re.findall(r"^int (crc32c_\w+)\(([^;]*)\);", header, re.M)
    batch = {name for name, params in decls
             if "crc32c_spans" in params or re.search(r"\bunsigned(\s+int)?\s+flags\b", params)}
    assert len(batch) == 13 and hic.ENTRY in batch
    mine, theirs = {op.entry for op in OPS}, {op.entry for op in ic.table()}
    assert mine == {hic.ENTRY} and not (mine & theirs)
    assert mine | theirs == batch
    # every parameter called flags, whatever its type, belongs to a counted declaration
    assert {name for name, params in decls if re.search(r"\bflags\b", params)} <= batch
    assert {op.where for op in OPS} == {"device", "host"}
    assert not ({op.name for op in OPS} & {op.name for op in ic.table()})


def test_expectations_are_self_consistent():
    for op in OPS:
        w, i = op.want, op.inputs
        for v in list(w.values()) + list(i.values()):
            if isinstance(v, np.ndarray):
                assert not v.flags.writeable
        n = i["offsets"].size
        if op.error:
            assert w["rc"] == ic.EWORK and w["nrepaired"] == w["nbad"] == 0 and np.array_equal(w["buf"], i["buf"])
            continue
        for key, size in (("ok", 1), ("bit", 8), ("lens", 4)):
            assert w[key].size == n + 1 and w[key][-1] == ic.SENT[size]
        ok, bit, lens = w["ok"][:-1], w["bit"][:-1], w["lens"][:-1]
        assert w["nrepaired"] == int((ok == 5).sum()) > 0 and w["nbad"] == int((ok == 0).sum())
        assert ((lens != 0) == (ok != 0)).all() and ((bit != 2**64 - 1) == (ok == 5)).all()
        changed = np.flatnonzero(w["buf"] != i["buf"])
        if i["flags"] & ic.LOCATE_ONLY:
            assert changed.size == 0
        else:  # one byte per repaired header, at the bit the call names
            want = sorted(int(o) + int(b) // 8 for o, b, v in zip(i["offsets"], bit, ok) if v == 5)
            assert changed.tolist() == want


def test_orders_with_the_header_ops_separate_errors():
    ops = list(ic.orders()["seed1"])
    mixed = []
    for j, op in enumerate(ops):
        mixed.append(op)
        if j % 3 == 2:
            mixed.append(OPS[(j // 3) % len(OPS)])
    mixed = ic.separate_errors(mixed)
    assert sum(op.entry == hic.ENTRY for op in mixed) >= 2 * len(OPS)
    for op, nxt in zip(mixed, mixed[1:] + [None]):
        if op.error:
            assert nxt is not None and not nxt.error and nxt.entry != op.entry, op.name
