"""The ops of crc32c_triage_pages for the out-of-order runs, made like those of
tests/interleave_cases.py (ic.Op: every expected array with the sentinel behind
it, each count, the return code) from the rule's model (tests/triage_model.py).
No GPU and no library call to build them; tests/test_gpu_interleave_triage.py
runs them among that table's ops, and tests/test_triage_interleave_cases.py
checks that the three tables together reach every batch entry point of
include/crc32c_batch.h."""
import functools

import numpy as np

from . import interleave_cases as ic
from . import raw_calls
from .raw_calls import _capped
from . import triage_cases as tc
from . import triage_model as tm

ENTRY = "crc32c_triage_pages"
COUNTS = raw_calls.TRIAGE_COUNTS


def _call_triage(op, side):
    i = op.inputs
    return ic._stated(op, raw_calls.listed_pages(ENTRY, side, i["buf"], i["wbuf"], cap=i["cap"]))


def _op(name, where, buf, W, cfl, short=0):
    """short: the capacity lies that many entries under the list's length."""
    assert cfl == 4
    m = tm.triage_fast(buf, W, cfl)
    cap = m["nitems"] - short if short else m["nitems"] + 3
    want = {"rc": m["rc"], "offsets": _capped(m["offsets"], cap, np.uint64), "lens": _capped(m["lens"], cap, np.uint32),
            "kind": _capped(m["kind"], cap, np.uint8), "buf": buf.copy()}
    want.update((k, m[k]) for k in COUNTS)
    return ic.Op(name, ENTRY, where, {"buf": buf, "wbuf": W, "cap": cap}, want, _call_triage,
                 demand=buf.size // 64 + (0 if where == "device" else buf.size), kind="triage")


@functools.lru_cache(maxsize=None)
def table():
    """The triage ops, in a fixed order; the last one returns early."""
    cases = tc.built()
    ops = []
    for name in ("behind_nkey0", "many_rounds"):
        buf, W, cfl, _ = cases[name]
        for where in ("device", "host"):
            ops.append(_op(f"triage_{name}_{where}", where, buf, W, cfl))
    buf, W, cfl, _ = cases["many_rounds"]
    ops.append(_op("triage_many_rounds_short_cap", "device", buf, W, cfl, short=5))
    buf, W, cfl, _ = cases["work_bound"]
    ops.append(_op("triage_over_the_work_bound", "device", buf, W, cfl))
    assert ops[-1].error and ops[-1].want["rc"] == ic.EWORK and not any(op.error for op in ops[:-1])
    assert all(op.want["nsuspect"] > 0 for op in ops[:-1]) and ops[-1].want["nsuspect"] == 0
    assert len({op.name for op in ops}) == len(ops)
    return tuple(ops)
