"""The ops of crc32c_repair_headers for the out-of-order runs, made like those
of tests/interleave_cases.py (ic.Op: every expected array with the sentinel
behind it, each count, each return code, the whole buffer afterwards) from the
rule's model (tests/header_model.py).  No GPU and no library call to build
them; tests/test_gpu_interleave_headers.py runs them among that table's ops and
tests/test_header_interleave_cases.py checks that the two tables together
reach every batch entry point of include/crc32c_batch.h."""
import functools

import numpy as np

from . import header_cases as hc
from . import header_model as hm
from . import interleave_cases as ic
from . import raw_calls
from . import salvage_cases as sc
from .repair_cases import flip, place

ENTRY = "crc32c_repair_headers"


def _call_headers(op, side):
    i = op.inputs
    got = raw_calls.repair_headers(side, i["buf"], i["offsets"], locate_only=bool(i["flags"] & ic.LOCATE_ONLY))
    return ic._stated(op, got, i["offsets"].size)


@functools.lru_cache(maxsize=None)
def table():
    """The header ops, in a fixed order; the last one returns early."""
    ops = []
    buf, offs, _bits, _nts = hc.packed(np.random.default_rng(8))
    offs = offs[::3].copy()
    for mode, flags in (("in_place", 0), ("locate_only", ic.LOCATE_ONLY)):
        ok, bit, lens, nrep, nbad, after = hm.repair(buf, offs, locate_only=bool(flags))
        assert nrep > 400 and nbad == 0
        want = {"rc": ic.OK, "ok": ic.ended(ok, np.uint8), "bit": ic.ended(bit, np.uint64),
                "lens": ic.ended(lens, np.uint32), "nrepaired": nrep, "nbad": nbad, "buf": after}
        for where in ("device", "host"):
            ops.append(ic.Op(f"headers_{mode}_{where}", ENTRY, where, {"buf": buf, "offsets": offs, "flags": flags},
                             want, _call_headers, demand=24 * 43 * offs.size + (0 if where == "device" else buf.size),
                             kind="headers"))
    # one damaged header of a 100 000-byte image listed 40 times: its true variant's spans pass 8 x base_bytes
    rng = np.random.default_rng(6)
    nt = 100000
    big, at = place([sc.image_nt(rng, nt), sc.image_nt(rng, 110000), sc.image_nt(rng, 110000)], lead=11)
    flip(big, int(at[0]), 256 + 3)
    assert 40 * (nt - 32) > hm.WORK_MAX * big.size
    want = {"rc": ic.EWORK, "nrepaired": 0, "nbad": 0, "buf": big.copy(), "ok_end": ic.SENT[1], "bit_end": ic.SENT[8],
            "lens_end": ic.SENT[4]}
    ops.append(ic.Op("headers_one_header_40_times", ENTRY, "device",
                     {"buf": big, "offsets": np.full(40, at[0], np.uint64), "flags": 0}, want, _call_headers,
                     demand=big.size, kind="headers"))
    assert len({op.name for op in ops}) == len(ops)
    return tuple(ops)
