"""The rule of CRC32C_SCRUB_GAPS (include/crc32c_batch.h) restated: the loop of
tests/scrub_model.py with the two lists built as the contract's header_list'
and item_list', over the models of the calls it composes (triage_model,
header_model, repair_model) and salvage_model.sane.  Nothing here comes from
the library.

``scrub(buf, W, ..., gaps=False)`` runs the same loop over scrub_model's two
lists and must equal scrub_model.scrub."""
from tests import salvage_model as sm
from tests import scrub_model as scm
from tests import triage_model as tm

GAPS = 0x40  # CRC32C_SCRUB_GAPS
COUNTS = scm.COUNTS


def gap_starts(offs, lens, kind, nbytes, W):
    """The end of every kind-4 entry that is no entry's offset and has 48
    bytes of the entry's own piece behind it, ascending, each once."""
    have, out = set(offs), []
    for o, ln, k in zip(offs, lens, kind):
        e = o + ln
        if k == tm.SALVAGED and e not in have and sm.piece_end(o, W, nbytes) - e >= 48:
            out.append(e)
    return sorted(set(out))


def header_list(offs, lens, kind, nbytes, W):
    """header_list': header_list(T) and gap_starts(T), ascending, each once."""
    return sorted(set(scm.header_list(offs, lens, kind, nbytes, W)) | set(gap_starts(offs, lens, kind, nbytes, W)))


def item_list(offs, lens, kind, buf, W, cfl=4):
    """item_list': item_list over T with every sane gap start merged in by
    offset as a suspect of its ITEM_ntotal."""
    buf = sm._u8(buf)
    extra = [(g, sm.sane(buf, W, g, cfl), tm.SUSPECT) for g in gap_starts(offs, lens, kind, len(buf), W)]
    merged = sorted(list(zip(offs, lens, kind)) + [e for e in extra if e[1]])
    return scm.item_list([e[0] for e in merged], [e[1] for e in merged], [e[2] for e in merged])


def first_lists(buf, W, cfl=4, gaps=True):
    """(header list, item list, suspects, gap starts) of the page's first triage."""
    T = tm.triage_fast(buf, W, cfl)
    args = T["offsets"], T["lens"], T["kind"]
    if not gaps:
        return scm.header_list(*args, len(buf), W), scm.item_list(*args), T["suspects"], []
    return (header_list(*args, len(buf), W), item_list(*args, buf, W, cfl), T["suspects"],
            gap_starts(*args, len(buf), W))


def scrub(buf, W, cfl=4, max_span=0, max_rounds=0, gaps=False, triage=tm.triage_fast):
    """The contract's loop, scrub_model.scrub's result dict; with ``gaps`` over the two lists above."""
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
        headers = header_list(*args, len(buf), W) if gaps else scm.header_list(*args, len(buf), W)
        rc, flips = scm._headers(buf, headers, W, cfl)
        if rc != scm.OK:
            break
        by = scm.BY_HEADER
        if not flips:
            items = item_list(*args, buf, W, cfl) if gaps else scm.item_list(*args)
            rc, flips = scm._items(buf, items, W, cfl, max_span)
            if rc != scm.OK:
                break
            by = scm.BY_ITEM
            if not flips:
                complete = 1
                break
        log += [(o, b, by) for o, b in flips]
        nh += len(flips) if by == scm.BY_HEADER else 0
        ni += len(flips) if by == scm.BY_ITEM else 0
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
