"""The rule of crc32c_scrub_pages (include/crc32c_batch.h) restated: the
contract's loop over the models of the three calls it composes
(tests/triage_model.py, tests/header_model.py, tests/repair_model.py), with the
two list builders restated from the C of INTEGRATION.md sections 4f and 4g.
Nothing here comes from the library.

``scrub`` returns a dict: rc, the final triage result's lists and six counts,
the log as three lists, nflips, headers_repaired, items_repaired, rounds,
complete, and ``after``, the buffer with every logged bit inverted."""
import numpy as np

from tests import header_model as hm
from tests import repair_model as rm
from tests import salvage_model as sm
from tests import triage_model as tm

OK, EINVAL, EWORK = 0, -3, -7
BY_HEADER, BY_ITEM = 1, 2
ROUNDS_DEFAULT = 64
COUNTS = ("nitems", "nbad", "nsalvaged", "nsuspect", "scanned", "ncand")


def header_list(offs, lens, kind, nbytes, W):
    """Section 4f: per piece every kind-0 entry, then the piece's walk end."""
    todo, k, n = [], 0, len(offs)
    for ps in range(0, nbytes, W):
        pe = min(ps + W, nbytes)
        end, last = ps, -1
        while k < n and offs[k] < pe:
            if kind[k] not in (tm.SALVAGED, tm.SUSPECT):
                if kind[k] == 0:
                    todo.append(offs[k])
                last = kind[k]
                end = offs[k] + lens[k]
            k += 1
        if last != 0 and ps <= end <= pe and pe - end >= 48:
            todo.append(end)
    return todo


def item_list(offs, lens, kind):
    """Section 4g: the damaged sane entries and the suspects the filter keeps."""
    todo, j, kept_end, n = [], 0, 0, len(offs)
    for k in range(n):
        if kind[k] == 0 and lens[k] != 0:
            todo.append(offs[k])
        if kind[k] != tm.SUSPECT:
            continue
        j = max(j, k + 1)
        while j < n and kind[j] not in (1, tm.SALVAGED):
            j += 1
        nxt = offs[j] if j < n else 1 << 64
        end = offs[k] + lens[k]
        if end > nxt or offs[k] < kept_end:
            continue
        todo.append(offs[k])
        kept_end = end
    return todo


def _headers(buf, todo, W, cfl):
    """crc32c_repair_headers in place: (rc, flips)."""
    if hm.work(buf, todo, W, cfl) > hm.WORK_MAX * len(buf):
        return EWORK, []
    ok, bit, _, _, _, after = hm.repair(buf, todo, W, cfl)
    buf[:] = after
    return OK, [(int(o), int(b)) for o, s, b in zip(todo, ok.tolist(), bit.tolist()) if s == hm.REPAIRED]


def _items(buf, todo, W, cfl, max_span):
    """crc32c_repair_items in place: (rc, flips).  (The verdicts are those of
    the buffer as the call finds it; the model's asserts hold the lists to
    disjoint repairs.)"""
    if rm.work(buf, todo, W, cfl, max_span) > len(buf):
        return EWORK, []
    ok, bit, _, _, after = rm.repair(buf, todo, W, cfl, max_span)
    buf[:] = after
    return OK, [(int(o), int(b)) for o, s, b in zip(todo, ok.tolist(), bit.tolist()) if s == rm.REPAIRED]


def scrub(buf, W, cfl=4, max_span=0, max_rounds=0, single_pass=False, triage=tm.triage_fast):
    """``single_pass``: the documents' written-out flow instead -- header
    rounds until one repairs nothing, then the items once, never the headers
    again (what case 7 tells apart)."""
    buf = sm._u8(buf).copy()
    if max_span > rm.SPAN_MAX:
        return {"rc": EINVAL}
    max_rounds = max_rounds or ROUNDS_DEFAULT
    log, rounds, complete, rc = [], 0, 0, OK
    nh = ni = 0
    T = triage(buf, W, cfl) if len(buf) else None
    if T is None:
        T = dict(rc=OK, offsets=[], lens=[], kind=[], **{c: 0 for c in COUNTS})
        complete = 1
    items_done = False
    while not complete:
        if T["rc"] != OK:
            rc = T["rc"]
            break
        flips = []
        if not (single_pass and items_done):
            rc, flips = _headers(buf, header_list(T["offsets"], T["lens"], T["kind"], len(buf), W), W, cfl)
            if rc != OK:
                break
        if flips:
            log += [(o, b, BY_HEADER) for o, b in flips]
            nh += len(flips)
            rounds += 1
            T = triage(buf, W, cfl)
            if rounds == max_rounds:
                break
            continue
        if single_pass and items_done:
            complete = 1
            break
        rc, flips = _items(buf, item_list(T["offsets"], T["lens"], T["kind"]), W, cfl, max_span)
        if rc != OK:
            break
        items_done = True
        if not flips:
            complete = 1
            break
        log += [(o, b, BY_ITEM) for o, b in flips]
        ni += len(flips)
        rounds += 1
        T = triage(buf, W, cfl)
        if rounds == max_rounds:
            break
    if rc == OK:
        rc = T["rc"]
    out = {c: T[c] for c in COUNTS}
    out.update(rc=rc, offsets=list(T["offsets"]), lens=list(T["lens"]), kind=list(T["kind"]),
               flip_offsets=[f[0] for f in log], flip_bits=[f[1] for f in log], flip_by=[f[2] for f in log],
               nflips=len(log), headers_repaired=nh, items_repaired=ni, rounds=rounds, complete=complete, after=buf)
    return out


def replay(buf, m):
    """The damaged bytes with the log's bits inverted, in order."""
    buf = sm._u8(buf).copy()
    for o, k in zip(m["flip_offsets"], m["flip_bits"]):
        buf[o + k // 8] ^= 1 << (k % 8)
    return buf
