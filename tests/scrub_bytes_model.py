"""The rule of CRC32C_SCRUB_BYTES (include/crc32c_batch.h) restated: the loop
of tests/scrub_gaps_model.py with the contract's third stage -- the model of
crc32c_repair_bytes (tests/repair_bytes_model.py) over the list the item stage
just ran on, its repairs logged one entry per bit.  The lists, ``_headers`` and
``_items`` are scrub_model's and scrub_gaps_model's.  Nothing here comes from
the library.

``scrub(buf, W, ..., byte_rule=False)`` must equal scrub_gaps_model.scrub."""
from tests import repair_bytes_model as bm
from tests import salvage_model as sm
from tests import scrub_gaps_model as gm
from tests import scrub_model as scm
from tests import triage_model as tm

BYTES = 0x80  # CRC32C_SCRUB_BYTES
BY_BYTE = 3   # CRC32C_SCRUB_BY_BYTE
COUNTS = scm.COUNTS


def bspan(max_span):
    """The byte stage's span limit."""
    return min(max_span, bm.SPAN_DEFAULT) if max_span else bm.SPAN_DEFAULT


def _bytes(buf, todo, W, cfl, max_span):
    """crc32c_repair_bytes in place: (rc, [(offset, byte, mask)])."""
    span = bspan(max_span)
    if scm.rm.work(buf, todo, W, cfl, span) > len(buf):
        return scm.EWORK, []
    ok, byte, mask, _, _, after = bm.repair(buf, todo, W, cfl, span)
    buf[:] = after
    return scm.OK, [(int(o), int(p), int(m)) for o, s, p, m in zip(todo, ok.tolist(), byte.tolist(), mask.tolist())
                    if s == bm.REPAIRED]


def bits(repairs):
    """A byte stage's log entries: per image one (offset, bit) per set bit of its mask, ascending."""
    return [(o, 8 * p + b) for o, p, m in repairs for b in range(8) if m >> b & 1]


def scrub(buf, W, cfl=4, max_span=0, max_rounds=0, gaps=False, byte_rule=False, triage=tm.triage_fast):
    """The contract's loop, scrub_model.scrub's result dict."""
    buf = sm._u8(buf).copy()
    if max_span > scm.rm.SPAN_MAX:
        return {"rc": scm.EINVAL}
    max_rounds = max_rounds or scm.ROUNDS_DEFAULT
    log, rounds, complete, rc = [], 0, 0, scm.OK
    nh = ni = 0
    T = triage(buf, W, cfl) if len(buf) else None
    if T is None:
        T = dict(rc=scm.OK, offsets=[], lens=[], kind=[], **{c: 0 for c in COUNTS})
        complete = 1
    while not complete:
        if T["rc"] != scm.OK:
            rc = T["rc"]
            break
        args = T["offsets"], T["lens"], T["kind"]
        headers = gm.header_list(*args, len(buf), W) if gaps else scm.header_list(*args, len(buf), W)
        rc, flips = scm._headers(buf, headers, W, cfl)
        if rc != scm.OK:
            break
        by, images = scm.BY_HEADER, len(flips)
        if not flips:
            items = gm.item_list(*args, buf, W, cfl) if gaps else scm.item_list(*args)
            rc, flips = scm._items(buf, items, W, cfl, max_span)
            if rc != scm.OK:
                break
            by, images = scm.BY_ITEM, len(flips)
            if not flips and byte_rule:
                rc, repairs = _bytes(buf, items, W, cfl, max_span)  # (the same list: the item stage changed nothing)
                if rc != scm.OK:
                    break
                by, images, flips = BY_BYTE, len(repairs), bits(repairs)
            if not flips:
                complete = 1
                break
        log += [(o, b, by) for o, b in flips]
        nh += images if by == scm.BY_HEADER else 0
        ni += images if by != scm.BY_HEADER else 0
        rounds += 1
        T = triage(buf, W, cfl)
        if rounds == max_rounds:
            break
    if rc == scm.OK:
        rc = T["rc"]
    out = {c: T[c] for c in COUNTS}
    out.update(rc=rc, offsets=list(T["offsets"]), lens=list(T["lens"]), kind=list(T["kind"]),
               flip_offsets=[f[0] for f in log], flip_bits=[f[1] for f in log], flip_by=[f[2] for f in log],
               nflips=len(log), headers_repaired=nh, items_repaired=ni, rounds=rounds, complete=complete, after=buf)
    return out


def byte_runs(m):
    """The log's BY_BYTE entries as maximal runs of one image's one byte: [(offset, byte, [bits])]."""
    runs = []
    for o, k, by in zip(m["flip_offsets"], m["flip_bits"], m["flip_by"]):
        if by != BY_BYTE:
            runs.append(None)  # (a run does not go on across another stage's entry)
        elif runs and runs[-1] and runs[-1][:2] == (o, k // 8):
            runs[-1][2].append(k % 8)
        else:
            runs.append((o, k // 8, [k % 8]))
    return [r for r in runs if r]
