"""Pages for the CRC32C_SCRUB_BYTES tests (no GPU, no library call): the CPU
model tests and the GPU tests share them.  Pieces of 2 to 16 KiB and images of
60 to 600 bytes, but for the span-limit pages (pieces of 128 KiB: the limit is
65 536 bytes); each case is the smallest page at which one step of the rule can
go wrong.

    name -> (buf, W, cfl, kwargs of the model's scrub without ``gaps``, notes)

Every case runs with CRC32C_SCRUB_GAPS and without.  notes: scrub_cases' keys
(checked for both, or with ``gaps_only`` only with the bit), and
    by           the log's flip_by sequence, exactly
    back         (offset, ntotal) of the images the flow must bring back:
                 equal to ``pristine`` over their whole length
    lost         (offset, ntotal) of damaged images that must stay as damaged
    pristine     the page before any damage."""
import numpy as np

from tests import salvage_cases as sc
from tests import scrub_cases as sca
from tests.repair_cases import flip

K2, K4, K16, K128 = 2 << 10, 4 << 10, 16 << 10, 128 << 10
ON = {"byte_rule": True}
TWO = 0x14  # bits 2 and 4 of one byte


def hit(buf, o, p, m=TWO):
    """Image byte p of the image at o XORed with mask m."""
    buf[o + p] ^= m


def _log(o, p, m, by=3):
    return [(o, 8 * p + b, by) for b in range(8) if m >> b & 1]


def reached(cfl=4):
    """The issue's page: two bits of one value byte of a walk-reached image."""
    rng = np.random.default_rng(1401)
    buf, offs = sc.pack([sca._imgs(rng, [200, 333, 600, 128], cfl, 2 if cfl == 8 else 0), sca._imgs(rng, [250, 90], cfl)],
                        K4)
    pristine, o = buf.copy(), offs[0]
    hit(buf, o[1], 100)
    return buf, K4, cfl, ON, {"rounds": 1, "headers_repaired": 0, "items_repaired": 1, "nflips": 2, "complete": 1,
                              "log": _log(o[1], 100, TWO), "final": {o[1]: 1}, "pristine": pristine,
                              "back": [(o[1], 333)]}


def reached_off():
    """The same page with the bit clear: the image stays lost."""
    buf, W, cfl, _, notes = reached()
    o = notes["back"][0][0]
    return buf, W, cfl, {}, {"rounds": 0, "nflips": 0, "complete": 1, "final": {o: 0}, "pristine": notes["pristine"],
                             "back": [], "lost": [(o, 333)]}


def suspect():
    """The same damage on a suspect: image 3 behind the dead image 1."""
    rng = np.random.default_rng(1402)
    buf, offs = sc.pack([sca._imgs(rng, [300, 359, 222, 500, 140]), sca._imgs(rng, [100, 200])], K4)
    pristine, o = buf.copy(), offs[0]
    sca._dead(buf, o[1])
    hit(buf, o[3], 100)
    return buf, K4, 4, ON, {"rounds": 1, "headers_repaired": 0, "items_repaired": 1, "complete": 1,
                            "log": _log(o[3], 100, TWO), "final": {o[3]: 4, o[2]: 4, o[4]: 4}, "absent": [o[1]],
                            "first_suspects": [o[3]], "pristine": pristine, "back": [(o[3], 500)]}


def gap_start():
    """Image 3, behind the intact image 2 behind the dead image 1, with two
    bits of its last byte inverted: no CRLF, so no candidate of the scan; with
    CRC32C_SCRUB_GAPS its offset is a gap start, and the byte stage's."""
    rng = np.random.default_rng(1403)
    nts = [200, 359, 150, 400, 90, 260, 120]
    buf, offs = sc.pack([sca._imgs(rng, nts), sca._imgs(rng, [100])], K4)
    pristine, o = buf.copy(), offs[0]
    sca._dead(buf, o[1])
    hit(buf, o[3], 399, 0x03)
    return buf, K4, 4, ON, {"gaps_only": True, "rounds": 1, "headers_repaired": 0, "items_repaired": 1, "complete": 1,
                            "log": _log(o[3], 399, 0x03), "final": {o[3]: 4, o[2]: 4, o[4]: 4}, "absent": [o[1]],
                            "first_suspects": [], "pristine": pristine, "back": [(o[3], 400)]}


def stage_order(max_rounds=0):
    """Image 1's nbytes bit 20 inverted, image 2 with one data bit, image 3
    with a byte hit, image 4's nkey 1 -> 0 (a length bit: the walk ends there,
    and the walk end is listed only once image 3 is good): headers, items,
    bytes, and the headers again."""
    rng = np.random.default_rng(1404)
    buf, offs = sc.pack([sca._imgs(rng, [100, 250, 330, 180, 70 * 7, 160]), sca._imgs(rng, [90])], K4)
    pristine, o = buf.copy(), offs[0]
    flip(buf, o[1], sca.GROW)
    flip(buf, o[2], sca.DATA)
    hit(buf, o[3], 77)
    assert buf[o[4] + 41] == 1
    flip(buf, o[4], 328)
    log = [(o[1], sca.GROW, 1), (o[2], sca.DATA, 2)] + _log(o[3], 77, TWO) + [(o[4], 328, 1)]
    if max_rounds:
        return buf, K4, 4, dict(ON, max_rounds=3), {
            "rounds": 3, "headers_repaired": 1, "items_repaired": 2, "nflips": 4, "complete": 0, "rc": 0,
            "log": log[:4], "by": [1, 2, 3, 3], "pristine": pristine,
            "back": [(o[i], n) for i, n in ((1, 250), (2, 330), (3, 180))],
            "lost": [(o[4], 490)]}
    return buf, K4, 4, ON, {"rounds": 4, "headers_repaired": 2, "items_repaired": 2, "nflips": 5, "complete": 1,
                            "log": log, "by": [1, 2, 3, 3, 1], "final": {o[i]: 1 for i in (1, 2, 3, 4, 5)},
                            "pristine": pristine,
                            "back": [(o[i], n) for i, n in ((1, 250), (2, 330), (3, 180), (4, 490))]}


def all_masks():
    """Image 1 with all eight bits of a byte inverted, image 2 with one bit of
    a byte: that one is the item stage's, logged so, a round earlier."""
    rng = np.random.default_rng(1405)
    buf, offs = sc.pack([sca._imgs(rng, [120, 480, 333, 90])], K2)
    pristine, o = buf.copy(), offs[0]
    hit(buf, o[1], 200, 0xFF)
    hit(buf, o[2], 150, 0x40)
    return buf, K2, 4, ON, {"rounds": 2, "headers_repaired": 0, "items_repaired": 2, "nflips": 9, "complete": 1,
                            "log": _log(o[2], 150, 0x40, 2) + _log(o[1], 200, 0xFF), "by": [2] + [3] * 8,
                            "final": {o[1]: 1, o[2]: 1}, "pristine": pristine, "back": [(o[1], 480), (o[2], 333)]}


EXCLUDED = [(32, 0x03), (33, TWO), (34, TWO), (35, 0x60), (41, 0x03), (38, 0x03), (39, 0x03)]
ALLOWED = [(38, 0x05), (39, 0x06), (40, TWO), (36, TWO)]


def excluded():
    """One piece per damaged image, the first of its piece: bytes 32..35 and
    41, byte 38 with bit 1 and byte 39 with bit 0 in the mask are not repaired;
    bytes 38 and 39 without those bits, and the bytes beside them, are."""
    rng = np.random.default_rng(1406)
    hits = EXCLUDED + ALLOWED
    buf, offs = sc.pack([sca._imgs(rng, [303 + 7 * i, 150, 99]) for i in range(len(hits))], K2)
    pristine = buf.copy()
    for (p, m), o in zip(hits, offs):
        hit(buf, o[0], p, m)
    back = [(o[0], 303 + 7 * i) for i, o in enumerate(offs) if i >= len(EXCLUDED)]
    return buf, K2, 4, ON, {"rounds": 1, "headers_repaired": 0, "items_repaired": len(ALLOWED), "complete": 1,
                            "by": [3] * sum(bin(m).count("1") for _, m in ALLOWED), "pristine": pristine,
                            "back": back, "lost": [(o[0], 303 + 7 * i) for i, o in enumerate(offs[:len(EXCLUDED)])]}


def stored_crc():
    """Two bits of a stored-CRC byte (image byte 29), and in a second image a
    bit of each of two neighbouring bytes: no one-byte error."""
    rng = np.random.default_rng(1407)
    buf, offs = sc.pack([sca._imgs(rng, [120, 480, 333, 90])], K2)
    pristine, o = buf.copy(), offs[0]
    hit(buf, o[1], 29)
    hit(buf, o[2], 150, 0x10)
    hit(buf, o[2], 151, 0x10)
    return buf, K2, 4, ON, {"rounds": 1, "headers_repaired": 0, "items_repaired": 1, "complete": 1,
                            "log": _log(o[1], 29, TWO), "final": {o[1]: 1, o[2]: 0}, "pristine": pristine,
                            "back": [(o[1], 480)], "lost": [(o[2], 333)]}


def span_limit(max_span=0):
    """Pieces of 128 KiB: a span of exactly 65 536 bytes is repaired, one of
    65 537 is not, whether max_span is 0 or far above the byte stage's cap."""
    rng = np.random.default_rng(1408)
    a, b = 32 + 0x10000, 32 + 0x10001
    buf, offs = sc.pack([[sc.image_nt(rng, a), sc.image_nt(rng, 200)], [sc.image_nt(rng, b), sc.image_nt(rng, 150)]],
                        K128, total=K128 + b + 150 + 100)
    pristine = buf.copy()
    hit(buf, offs[0][0], 40000)
    hit(buf, offs[1][0], 40000)
    return buf, K128, 4, dict(ON, max_span=max_span), {
        "rounds": 1, "headers_repaired": 0, "items_repaired": 1, "complete": 1, "log": _log(0, 40000, TWO),
        "final": {0: 1, K128: 0}, "pristine": pristine, "back": [(0, a)], "lost": [(K128, b)]}


def span_300():
    """max_span = 300 caps the byte stage as it caps the item stage."""
    rng = np.random.default_rng(1409)
    buf, offs = sc.pack([sca._imgs(rng, [120, 332, 333, 90])], K2)
    pristine, o = buf.copy(), offs[0]
    hit(buf, o[1], 100)
    hit(buf, o[2], 100)
    return buf, K2, 4, dict(ON, max_span=300), {
        "rounds": 1, "headers_repaired": 0, "items_repaired": 1, "complete": 1, "log": _log(o[1], 100, TWO),
        "final": {o[1]: 1, o[2]: 0}, "pristine": pristine, "back": [(o[1], 332)], "lost": [(o[2], 333)]}


LOG_HITS = (0, 500, 1022, 1023, 1024, 1025, -1)  # indices of the item list


def log_rounds():
    """1 100 walked images of 60 to 64 bytes (scrub_cases' sizes: images of one
    size all end where a grown length would, and the header stage's work bound
    ends the flow), every one damaged, so every one is on the item list: a bit
    of each of two bytes (nobody's to repair), but for seven images with a
    byte hit, on both sides of list index 1 024 and in k_scrub_log_bytes'
    last, partial round."""
    from tests import scrub_model as scm
    from tests import triage_model as tm
    rng = np.random.default_rng(1410)
    per = [256, 256, 256, 256, 76]
    buf, offs = sc.pack([sca._sixty(rng, m) for m in per], K16)
    pristine = buf.copy()
    flat = [o for piece in offs for o in piece]
    for o in flat:
        hit(buf, o, 56, 0x10)
        hit(buf, o, 57, 0x10)

    def items():
        T = tm.triage_fast(buf, K16, 4)
        return scm.item_list(T["offsets"], T["lens"], T["kind"])

    first = items()  # (the images, and a few look-alikes in their bytes)
    assert set(flat) <= set(first) and len(first) > 1024 + 64
    chosen = [first[i] for i in LOG_HITS[:-1]] + [first[-1]]
    assert set(chosen) <= set(flat)
    log = []
    for o, m in zip(chosen, [0x03, 0xFF, 0x81, 0x7E, 0x18, 0xC0, 0x2C]):
        hit(buf, o, 56, 0x10 ^ m)
        hit(buf, o, 57, 0x10)
        log += _log(o, 56, m)
    assert items() == first
    return buf, K16, 4, ON, {"rounds": 1, "headers_repaired": 0, "items_repaired": len(chosen), "nflips": len(log),
                             "complete": 1, "log": log, "first_items_n": len(first), "pristine": pristine,
                             "back": [(o, 60) for o in chosen]}


CASES = {
    "reached": reached, "reached_off": reached_off, "suspect": suspect, "gap_start": gap_start,
    "stage_order": stage_order, "stage_order_three_rounds": lambda: stage_order(3), "all_masks": all_masks,
    "excluded": excluded, "stored_crc": stored_crc, "span_limit": span_limit,
    "span_limit_max_span_2_20": lambda: span_limit(1 << 20), "span_300": span_300, "log_rounds": log_rounds,
    "cflags64": lambda: reached(8),
}
_BUILT = {}


def case(name):
    """The case, built once."""
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]


def check_notes(m, first, notes, damaged, gaps):
    """scrub_cases.check_notes and this file's own keys: m the scrub's result
    dict, first = (header list, item list, suspects) of the damaged page's
    first triage, damaged the page as the scrub found it."""
    if gaps or not notes.get("gaps_only"):
        sca.check_notes(m, first, notes)
        if "by" in notes:
            assert m["flip_by"] == notes["by"], m["flip_by"]
        if "first_items_n" in notes:
            assert len(first[1]) == notes["first_items_n"]
        for o, nt in notes["back"]:
            assert (m["after"][o:o + nt] == notes["pristine"][o:o + nt]).all(), o
    for o, nt in notes.get("lost", ()):
        assert (m["after"][o:o + nt] == damaged[o:o + nt]).all(), o
        assert (damaged[o:o + nt] != notes["pristine"][o:o + nt]).any(), o
