"""The ops of crc32c_scrub_pages for the out-of-order runs, made like those of
tests/interleave_cases.py (ic.Op: every expected array with the sentinel behind
it, each count, the return code, the page afterwards) from the rule's model
(tests/scrub_model.py) over pages of tests/scrub_cases.py.  No GPU and no
library call to build them; tests/test_gpu_interleave_scrub.py runs them among
that table's ops, and tests/test_scrub_interleave_cases.py checks that every
entry point taking a crc32c_scrub_opts is an entry here."""
import functools

from . import interleave_cases as ic
from . import raw_calls
from .raw_calls import _capped
from . import scrub_cases as sca
from . import scrub_model as scm

ENTRY = "crc32c_scrub_pages"
WORDS, LISTS = raw_calls.SCRUB_WORDS, raw_calls.SCRUB_LISTS
assert WORDS[:6] == scm.COUNTS


def _call_scrub(op, side):
    i = op.inputs
    got = raw_calls.scrub_pages(side, i["buf"], i["wbuf"], cap=i["cap"], flip_cap=i["flip_cap"],
                                max_rounds=i["max_rounds"], locate_only=bool(i["mode"] & ic.LOCATE_ONLY))
    return ic._stated(op, got)


def _op(name, where, case, short=0, mode=0, max_rounds=0, refused=False):
    """short: both capacities lie that many entries under what is needed."""
    buf, W, cfl, kw, _ = sca.case(case)
    assert cfl == 4 and not kw
    m = scm.scrub(buf, W, cfl, max_rounds=max_rounds)
    cap, flip_cap = (max(m["nitems"] - short, 0), max(m["nflips"] - short, 0)) if short else (m["nitems"] + 3,
                                                                                               m["nflips"] + 2)
    if refused:  # (a device page with CRC32C_LOCATE_ONLY: nothing is written, not even the counts)
        want = {"rc": ic.EINVAL, "buf": buf.copy()}
        want.update((n, _capped([], room, d)) for (n, d), room in zip(LISTS, [cap] * 3 + [flip_cap] * 3))
        want.update((w, ic.SENT[4] if w in ("rounds", "complete") else ic.SENT64) for w in WORDS)
    else:
        want = {"rc": m["rc"], "buf": buf.copy() if mode & ic.LOCATE_ONLY else m["after"].copy()}
        want.update((n, _capped(m[n], room, d)) for (n, d), room in zip(LISTS, [cap] * 3 + [flip_cap] * 3))
        want.update((w, m[w]) for w in WORDS)
    return ic.Op(name, ENTRY, where, {"buf": buf, "wbuf": W, "cap": cap, "flip_cap": flip_cap, "mode": mode,
                                      "max_rounds": max_rounds}, want, _call_scrub,
                 demand=buf.size // 8 + (0 if where == "device" else buf.size), kind="scrub")


@functools.lru_cache(maxsize=None)
def table():
    """The scrub ops, in a fixed order; the last two return early, one before
    it touches the device and one behind the first triage's scan."""
    ops = []
    for case in ("second_pass", "suspects_per_piece"):
        for where in ("device", "host"):
            ops.append(_op(f"scrub_{case}_{where}", where, case))
    ops.append(_op("scrub_two_rounds_short_caps", "device", "two_rounds", short=1))
    ops.append(_op("scrub_two_rounds_one_round", "host", "two_rounds", max_rounds=1))
    ops.append(_op("scrub_second_pass_locate_only", "host", "second_pass", mode=ic.LOCATE_ONLY))
    ops.append(_op("scrub_locate_only_on_a_device_page", "device", "second_pass", mode=ic.LOCATE_ONLY, refused=True))
    ops.append(_op("scrub_over_the_work_bound", "device", "work_bound"))
    assert ops[-1].want["rc"] == ic.EWORK and ops[-2].error and not any(op.error for op in ops[:-2])
    assert all(op.want["nflips"] > 0 for op in ops[:-2])
    assert len({op.name for op in ops}) == len(ops)
    return tuple(ops)
