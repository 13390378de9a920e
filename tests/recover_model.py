"""The rule of crc32c_recover_pages (include/crc32c_batch.h) restated over
numpy: the composition of the walk (salvage_cases.walk_lists), the salvage over
its lists (salvage_model.salvage_fast) and the header rule
(salvage_model.sane).  Nothing here comes from the library."""
import numpy as np

from tests import salvage_cases as sc
from tests import salvage_model as sm

SALVAGED = 4  # CRC32C_ITEM_SALVAGED
OK, EWORK = 0, -7


def many_found():
    """Three 64 KiB wbufs: 270 images of 60-260 B between two sparse wbufs, one
    nbytes bit of the middle wbuf's image 2 flipped.  The walk of that piece
    stops after four entries and the salvage finds every image behind the
    damaged one: more than four rounds of 64 in one piece, the lists
    interleaved."""
    rng = np.random.default_rng(700)
    first = sc.mixed(rng, sc.K64, 0.2)
    imgs = [sc.image_nt(rng, int(rng.integers(60, 261))) for _ in range(270)]
    buf, offs = sc.pack([first, imgs, sc.mixed(rng, sc.K64, 0.2)], sc.K64)
    sc.HEADER_DAMAGE["nbytes_b0"](buf, offs[1][2])
    return buf, sc.K64, 4


def work_bound_behind_a_walk():
    """salvage_cases.work_bound_case() (whose only wbuf's walk ends at its first
    byte) behind a full, intact wbuf: past the work bound with a walk's part
    that is not empty."""
    buf, W = sc.work_bound_case()
    front, _ = sc.pack([sc.mixed(np.random.default_rng(301), W, 1.0)], W)
    return np.concatenate((front, buf)), W


def recover(buf, W, cfl=4):
    """A dict of what crc32c_recover_pages returns with room for every entry:
    rc, offsets, lens, kind (lists), nitems, nbad, nsalvaged, scanned, ncand;
    and the two lists it is made of (walked, wok, found)."""
    walked, wok = sc.walk_lists(buf, W, cfl)
    found, scanned, ncand, work = sm.salvage_fast(buf, W, walked, wok, cfl)
    rc = OK
    if work > sm.WORK_MAX * (scanned + W):
        rc, found = EWORK, []
    entries = [(int(o), int(k)) for o, k in zip(walked.tolist(), wok.tolist())] + [(o, SALVAGED) for o in found]
    entries.sort()
    offsets = [o for o, _ in entries]
    return {
        "rc": rc, "offsets": offsets, "kind": [k for _, k in entries],
        "lens": [sm.sane(sm._u8(buf), W, o, cfl) for o in offsets],
        "nitems": len(entries), "nbad": int((wok == 0).sum()), "nsalvaged": len(found), "scanned": scanned,
        "ncand": ncand, "walked": walked, "wok": wok, "found": found,
    }
