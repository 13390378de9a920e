"""The rule of crc32c_triage_pages (include/crc32c_batch.h) restated over numpy
on top of the salvage's model (tests/salvage_model.py) and the walk
(salvage_cases.walk_lists).  Nothing here comes from the library.

Two versions that must agree: ``triage_bytewise`` is the four-line rule as
written, one offset at a time; ``triage_fast`` goes through the candidate list
only.  Both return the dict ``recover_model.recover`` returns, with the
suspects merged in (kind 6) and ``nsuspect`` / ``suspects`` beside it."""
import numpy as np

from tests import oracle
from tests import salvage_cases as sc
from tests import salvage_model as sm

SALVAGED, SUSPECT = 4, 6  # CRC32C_ITEM_SALVAGED, CRC32C_ITEM_SUSPECT
OK, EWORK = 0, -7


def _result(buf, W, cfl, walked, wok, found, suspects, scanned, ncand, rc):
    entries = [(int(o), int(k)) for o, k in zip(walked.tolist(), wok.tolist())]
    entries += [(o, SALVAGED) for o in found] + [(o, SUSPECT) for o in suspects]
    entries.sort()
    offsets = [o for o, _ in entries]
    return {
        "rc": rc, "offsets": offsets, "kind": [k for _, k in entries],
        "lens": [sm.sane(buf, W, o, cfl) for o in offsets],
        "nitems": len(entries), "nbad": int((wok == 0).sum()), "nsalvaged": len(found), "nsuspect": len(suspects),
        "scanned": scanned, "ncand": ncand, "walked": walked, "wok": wok, "found": found, "suspects": suspects,
    }


def triage_bytewise(buf, W, cfl=4):
    buf = sm._u8(buf)
    n = len(buf)
    walked, wok = sc.walk_lists(buf, W, cfl)
    is_walked = set(walked.tolist())
    cov = sm.covered_mask(buf, W, walked, wok, cfl)
    scanned = ncand = work = 0
    for o in range(n):
        if sm.piece_end(o, W, n) - o >= 48 and not cov[o]:
            scanned += 1
            nt = sm.candidate(buf, W, o, cfl)
            if nt:
                ncand += 1
                work += nt - 32
    if work > sm.WORK_MAX * (scanned + W):
        return _result(buf, W, cfl, walked, wok, [], [], scanned, ncand, EWORK)
    found, suspects = [], []
    for ps in range(0, n, W):
        pe, o = min(ps + W, n), ps
        while pe - o >= 48:
            if cov[o]:
                o += 1  # (to the end of the covering image, one covered byte at a time)
            elif sm.intact(buf, W, o, cfl):
                found.append(o)
                o += sm.intact(buf, W, o, cfl)
            elif sm.candidate(buf, W, o, cfl) and o not in is_walked:
                suspects.append(o)
                o += 1
            else:
                o += 1
    return _result(buf, W, cfl, walked, wok, found, suspects, scanned, ncand, OK)


def triage_fast(buf, W, cfl=4):
    buf = sm._u8(buf)
    walked, wok = sc.walk_lists(buf, W, cfl)
    is_walked = set(walked.tolist())
    cov = sm.covered_mask(buf, W, walked, wok, cfl)
    offs, nts, scanned = sm._candidates_fast(buf, W, cov, cfl)
    if int((nts - 32).sum()) > sm.WORK_MAX * (scanned + W):
        return _result(buf, W, cfl, walked, wok, [], [], scanned, len(offs), EWORK)
    found, suspects = [], []
    end = 0  # (images stay inside their piece, so one running end serves every piece)
    for o, nt in zip(offs.tolist(), nts.tolist()):
        if o < end:
            continue
        stored = int.from_bytes(bytes(buf[o + 28:o + 32]), "little")
        if oracle.crc32c(0, buf[o + 32:o + nt]) == stored:
            found.append(o)
            end = o + nt
        elif o not in is_walked:
            suspects.append(o)
    return _result(buf, W, cfl, walked, wok, found, suspects, scanned, len(offs), OK)


def without_suspects(m):
    """The lists and counts of a triage result (model dict) with the kind-6
    entries taken out: what crc32c_recover_pages returns."""
    keep = [i for i, k in enumerate(m["kind"]) if k != SUSPECT]
    out = {k: m[k] for k in ("rc", "nbad", "nsalvaged", "scanned", "ncand")}
    out.update({k: [m[k][i] for i in keep] for k in ("offsets", "lens", "kind")})
    out["nitems"] = len(keep)
    return out
