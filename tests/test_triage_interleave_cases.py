"""The triage ops of tests/triage_interleave_cases.py, checked without a GPU,
and the guard that goes with them: every function of include/crc32c_batch.h
that takes a batch is an entry of one of the three out-of-order tables --
tests/interleave_cases.py's, the header ops' or the triage ops', which
tests/test_gpu_interleave_triage.py runs among the first one's.

tests/test_interleave_cases.py pins the declarations that say `unsigned flags`
at its own twelve, and tests/test_header_interleave_cases.py every parameter
called flags at those and crc32c_repair_headers; crc32c_triage_pages therefore
calls its flags word call_flags.  This guard does not go by the spelling: a
function of any return type takes a batch when it has a crc32c_spans, an
identifier that ends in `flags`, or an `unsigned` word directly in front of
`void *stream`, and no count is pinned, so the next entry point needs a table
entry and no new name."""
import os
import re

import numpy as np

from tests import header_interleave_cases as hic
from tests import interleave_cases as ic
from tests import triage_interleave_cases as tic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = tic.table()


def _batch_entry_points():
    header = open(os.path.join(ROOT, "include", "crc32c_batch.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = re.findall(r"^[\w \*]*?\b(crc32c_\w+)\(([^;{]*)\);", header, re.M)
    names = {name for name, _ in decls}
    assert len(names) == len(decls)
    # whatever they return: int, a pointer, a word, a float, nothing
    assert {"crc32c_batch", "crc32c_strerror", "crc32c_host_alloc", "crc32c_locate_bit", "crc32c_last_kernel_ms",
            "crc32c_host_free"} <= names
    takes = re.compile(r"crc32c_spans|\w*flags\b|\bunsigned(\s+int)?\s+\w+\s*,\s*void\s*\*\s*stream")
    return {name for name, params in decls if takes.search(params)}


def test_the_three_tables_cover_every_batch_entry_point():
    batch = _batch_entry_points()
    theirs, headers, mine = ({op.entry for op in t} for t in (ic.table(), hic.table(), OPS))
    assert mine == {tic.ENTRY} and headers == {hic.ENTRY} and len(theirs) == 12
    assert not (mine & theirs) and not (mine & headers)
    assert theirs | headers | mine == batch
    assert {op.where for op in OPS} == {"device", "host"}
    assert not ({op.name for op in OPS} & ({op.name for op in ic.table()} | {op.name for op in hic.table()}))


def test_the_guard_sees_a_flags_word_under_any_name():
    """The entry point is found by what its declaration is, whatever it calls
    the word: its parameter list is crc32c_recover_pages' with nsuspect added
    and the word renamed."""
    header = open(os.path.join(ROOT, "include", "crc32c_batch.h")).read()
    params = {name: re.sub(r"\s+", " ", p) for name, p in re.findall(r"^int (crc32c_\w+)\(([^;]*)\);", header, re.M)}
    mine, recover = params[tic.ENTRY], params["crc32c_recover_pages"]
    assert not re.search(r"\bflags\b", mine)
    assert mine.replace("uint64_t *nsuspect, ", "").replace("unsigned call_flags", "unsigned flags") == recover


def test_expectations_are_self_consistent():
    for op in OPS:
        w, i = op.want, op.inputs
        for v in list(w.values()) + list(i.values()):
            if isinstance(v, np.ndarray):
                assert not v.flags.writeable
        assert np.array_equal(w["buf"], i["buf"])  # the call reads only
        cap, n = i["cap"], w["nitems"]
        k = min(cap, n)
        for key, size in (("offsets", 8), ("lens", 4), ("kind", 1)):
            assert w[key].size == cap + 1 and (w[key][k:] == ic.SENT[size]).all()
        offs, kind = w["offsets"][:k], w["kind"][:k]
        assert (np.diff(offs.astype(np.int64)) > 0).all()
        if op.error:
            assert w["rc"] == ic.EWORK and w["nsuspect"] == w["nsalvaged"] == 0 and not (kind >= 4).any()
            continue
        assert w["rc"] == 0 and set(kind.tolist()) <= {0, 1, 4, 6}
        if cap >= n:
            assert int((kind == 6).sum()) == w["nsuspect"] > 0 and int((kind == 4).sum()) == w["nsalvaged"]
            assert int((kind == 0).sum()) == w["nbad"]
        assert w["nsuspect"] <= w["ncand"] - w["nsalvaged"]


def test_orders_with_the_triage_ops_separate_errors():
    ops = list(ic.orders()["seed2"])
    mixed = []
    for j, op in enumerate(ops):
        mixed.append(op)
        if j % 3 == 2:
            mixed.append(OPS[(j // 3) % len(OPS)])
    mixed = ic.separate_errors(mixed)
    assert sum(op.entry == tic.ENTRY for op in mixed) >= 2 * len(OPS)
    for op, nxt in zip(mixed, mixed[1:] + [None]):
        if op.error:
            assert nxt is not None and not nxt.error and nxt.entry != op.entry, op.name
