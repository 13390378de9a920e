"""Pages for the CRC32C_SCRUB_GAPS tests (no GPU, no library call): the CPU
model tests and the GPU tests share them.  Pieces of 2 to 16 KiB, images of 60
to 600 bytes, at most 8 pieces; each case is the smallest page at which one
step of the rule can go wrong.

    name -> (buf, W, cfl, kwargs of the model's scrub, notes)

notes: scrub_cases' keys, and
    first_gaps     gap_starts of the damaged page's first triage, exactly
    first_items    its item list, exactly
    back           (offset, ntotal) of the images the flow must bring back:
                   proven in the final list and equal to ``pristine`` from
                   byte 28 on
    pristine       the page before any damage."""
import struct

import numpy as np

from tests import salvage_cases as sc
from tests import salvage_model as sm
from tests import scrub_cases as sca
from tests import triage_cases as tc
from tests.repair_cases import flip

K2, K4, K16 = 2 << 10, 4 << 10, 16 << 10
GROW = sca.GROW
ON = {"gaps": True}


def _crlf(nt):
    """Bit 1 of an image's last byte: "\\n" becomes 0x08."""
    return 8 * (nt - 1) + 1


def _plant(value, at, nt):
    """A sane header in a value's bytes at index ``at``: nkey 1, no CAS, no
    client flags, ITEM_ntotal nt."""
    struct.pack_into("<I", value, at + 32, nt - 50)
    value[at + 38:at + 40] = b"\0\0"
    value[at + 41] = 1


def behind(cfl=4, gaps=True):
    """The issue's page: image 1 dead, image 3 with nbytes bit 20 inverted,
    image 5 with bit 1 of its last byte inverted."""
    rng = np.random.default_rng(1301)
    nts = [200, 359, 150, 400, 90, 260, 120]
    buf, offs = sc.pack([sca._imgs(rng, nts, cfl, 2 if cfl == 8 else 0)], K4)
    pristine, o = buf.copy(), offs[0]
    sca._dead(buf, o[1])
    flip(buf, o[3], GROW)
    flip(buf, o[5], _crlf(260))
    assert (o[3], o[5]) == (709, 1199)
    if not gaps:
        return buf, K4, cfl, {}, {"rounds": 0, "nflips": 0, "complete": 1, "absent": [o[1], o[3], o[5]],
                                  "first_gaps": [], "pristine": pristine, "back": []}
    return buf, K4, cfl, ON, {"rounds": 2, "headers_repaired": 1, "items_repaired": 1, "complete": 1,
                              "log": [(709, 276, 1), (1199, 2073, 2)], "final": {o[3]: 4, o[5]: 4, o[2]: 4, o[6]: 4},
                              "absent": [o[1]], "first_gaps": [709, 1199, o[6] + 120],
                              "first_headers": [200, 709, 1199, o[6] + 120], "first_items": [1199],
                              "pristine": pristine, "back": [(o[3], 400), (o[5], 260)]}


def neighbour_of_dead():
    """A length-flipped image directly behind the dead header: no proven image
    ends where it starts."""
    rng = np.random.default_rng(1302)
    buf, offs = sc.pack([sca._imgs(rng, [200, 303, 250, 150, 100])], K2)
    pristine, o = buf.copy(), offs[0]
    sca._dead(buf, o[1])
    flip(buf, o[2], GROW)
    return buf, K2, 4, ON, {"rounds": 0, "nflips": 0, "complete": 1, "absent": [o[1], o[2]],
                            "final": {o[3]: 4, o[4]: 4}, "first_gaps": [o[4] + 100],
                            "first_headers": [o[1], o[4] + 100], "pristine": pristine, "back": []}


def chain(max_rounds=0):
    """Three consecutive length-flipped images behind an intact one, itself
    behind a dead header: each is the next one's proven predecessor only once
    repaired, one image a round."""
    rng = np.random.default_rng(1303)
    nts = [120, 303, 200, 150, 260, 99, 180]
    buf, offs = sc.pack([sca._imgs(rng, nts)], K2)
    pristine, o = buf.copy(), offs[0]
    sca._dead(buf, o[1])
    for i in (3, 4, 5):
        flip(buf, o[i], GROW)
    if max_rounds:
        return buf, K2, 4, dict(ON, max_rounds=2), {
            "rounds": 2, "headers_repaired": 2, "complete": 0, "rc": 0, "log": [(o[3], GROW, 1), (o[4], GROW, 1)],
            "final": {o[3]: 4, o[4]: 4}, "absent": [o[1], o[5]], "pristine": pristine,
            "back": [(o[3], 150), (o[4], 260)]}
    return buf, K2, 4, ON, {"rounds": 3, "headers_repaired": 3, "items_repaired": 0, "complete": 1,
                            "log": [(o[i], GROW, 1) for i in (3, 4, 5)], "final": {o[i]: 4 for i in (2, 3, 4, 5, 6)},
                            "absent": [o[1]], "first_gaps": [o[3], o[6] + 180], "pristine": pristine,
                            "back": [(o[3], 150), (o[4], 260), (o[5], 99)]}


def edge():
    """Behind a dead first image, the last salvaged image ends exactly 48 bytes
    before its piece's end in piece 0 (listed: the header there is zeros, its
    verdict 0), 47 bytes before it in piece 1 (not listed), and 48 bytes before
    the page's end in piece 2, which the page's end cuts short."""
    rng = np.random.default_rng(1304)
    a = sca._imgs(rng, [303, 500, 600, K2 - 48 - 1403])
    b = sca._imgs(rng, [310, 500, 600, K2 - 47 - 1410])
    c = sca._imgs(rng, [303, 349, 300])
    buf, offs = sc.pack([a, b, c], K2, total=2 * K2 + 1000)
    pristine = buf.copy()
    for o in offs:
        sca._dead(buf, o[0])
    gaps = [K2 - 48, 2 * K2 + 952]
    return buf, K2, 4, ON, {"rounds": 0, "nflips": 0, "complete": 1, "first_gaps": gaps,
                            "first_headers": [0, K2 - 48, K2, 2 * K2, 2 * K2 + 952], "first_items": [],
                            "pristine": pristine, "back": []}


def abutting():
    """Salvaged entries followed at once by a kind-0 entry (image 1, inside the
    span that image 0's grown length claims, ends where the walk goes on: at
    image 2, one data bit inverted), by a salvaged entry (image 4), by a
    suspect (image 5 ends at image 6, one data bit inverted) -- none of these
    ends is a gap start -- and by nothing (image 7)."""
    rng = np.random.default_rng(1305)
    nts = [200, 256, 180, 303, 150, 220, 333, 90]
    buf, offs = sc.pack([sca._imgs(rng, nts)], K2)
    pristine, o = buf.copy(), offs[0]
    assert not buf[o[0] + 33] & 1
    flip(buf, o[0], 256 + 8)  # nbytes + 256: image 0 now ends where image 1 does
    flip(buf, o[2], sca.DATA)
    sca._dead(buf, o[3])
    flip(buf, o[6], sca.DATA)
    end = o[7] + 90
    return buf, K2, 4, ON, {"complete": 1, "first_gaps": [end], "first_headers": [o[0], o[2], end],
                            "first_suspects": [o[6]], "first_items": [o[0], o[2], o[6]], "pristine": pristine,
                            "back": [(o[0], 200), (o[2], 180), (o[6], 333)], "absent": [o[3]]}


def entry_inside():
    """Image 0's nbytes bit 8 cleared: the walk goes on inside its value, where
    a planted sane header sends it into image 1's value, a second one from
    there into image 3's value and a third one onto zeros.  Images 1 and 3 are
    intact (salvaged), each with a walked kind-0 entry strictly inside.  Image
    2, behind image 1, has nbytes bit 20 inverted: image 1's end is a gap
    start although the entry behind image 1 in the list is not at that end.
    Image 3's end is image 4's offset, an entry, although the entry behind
    image 3 in the list is another: no gap start."""
    rng = np.random.default_rng(1306)
    p1, p2, p3, stop = 244, 500 + 150, 1200 + 100, 1900

    def img(nt, at=None, span=0):
        nkey = 1 + nt % 7
        value = bytearray(bytes(rng.integers(0, 256, nt - 51 - nkey, dtype=np.uint8)))
        if at is not None:
            _plant(value, at - 49 - nkey, span)
        return sc.image_nt(rng, nt, value=bytes(value))

    imgs = [img(500, p1, p2 - p1), img(400, 150, p3 - p2), img(300), img(450, 100, stop - p3), img(200)]
    buf, offs = sc.pack([imgs], K4)
    pristine, o = buf.copy(), offs[0]
    assert o == [0, 500, 900, 1200, 1650] and buf[o[0] + 33] & 1
    flip(buf, o[0], 256 + 8)
    flip(buf, o[2], GROW)
    assert sm.sane(buf, K4, 0) == p1 and sm.sane(buf, K4, p1) == p2 - p1 and sm.sane(buf, K4, p2) == p3 - p2
    assert sm.sane(buf, K4, p3) == stop - p3 and o[1] < p2 < o[2] and o[3] < p3 < o[4]
    return buf, K4, 4, ON, {"complete": 1, "first_gaps": [o[2], o[4] + 200],
                            "first_headers": [0, p1, p2, o[2], p3, o[4] + 200], "first_kinds": {p2: 0, p3: 0, o[1]: 4,
                                                                                              o[3]: 4, o[4]: 4},
                            "final": {o[0]: 1, o[2]: 1, o[4]: 1}, "pristine": pristine,
                            "back": [(o[0], 500), (o[2], 300)]}


def overlap():
    """Piece 0: image 3, behind the intact image 2, has bit 1 of its last byte
    inverted and holds a complete failing look-alike in its value -- a suspect:
    the gap start is kept and the suspect inside it dropped.  Piece 1: behind
    the intact image 1 lie 100 bytes of garbage under a sane header that
    claims 450, then the intact image 2: the gap start's span runs past a
    proven entry and is dropped."""
    rng = np.random.default_rng(1307)
    inner = tc._lookalike(rng, 200)
    value = bytes(rng.integers(0, 256, 50, dtype=np.uint8)) + bytes(inner) + bytes(
        rng.integers(0, 256, 60, dtype=np.uint8))
    outer = sc.stamp(sc.layout.make_item(b"xk", value, cas=None))
    nto = len(outer)
    garbage = bytearray(bytes(rng.integers(0, 256, 100, dtype=np.uint8)))
    _plant(garbage, 0, 450)
    a = sca._imgs(rng, [100, 303, 200]) + [outer] + sca._imgs(rng, [150])
    b = sca._imgs(rng, [247, 140]) + [garbage] + sca._imgs(rng, [400, 77])
    buf, offs = sc.pack([a, b], K2)
    pristine, o, q = buf.copy(), offs[0], offs[1]
    sca._dead(buf, o[1])
    sca._dead(buf, q[0])
    flip(buf, o[3], _crlf(nto))
    y, g = o[3] + 48 + 2 + 1 + 50, q[2]
    assert sm.candidate(buf, K2, y) == 200 and not sm.intact(buf, K2, y)
    assert sm.sane(buf, K2, g) == 450 and not sm.candidate(buf, K2, g) and q[3] == g + 100
    return buf, K2, 4, ON, {"rounds": 1, "items_repaired": 1, "headers_repaired": 0, "complete": 1,
                            "log": [(o[3], _crlf(nto), 2)], "first_suspects": [y],
                            "first_gaps": [o[3], o[4] + 150, g, q[4] + 77], "first_items": [o[3]],
                            "final": {o[3]: 4, q[3]: 4}, "absent": [y, g, o[1], q[0]], "pristine": pristine,
                            "back": [(o[3], nto)]}


def rounds_of_64():
    """Pieces with 63, 64 and 65 gap starts: a dead first image, then intact
    and length-flipped images in turn, around k_scrub_gaps' round of 64."""
    rng = np.random.default_rng(1308)
    wbufs = [sca._imgs(rng, [72]) + sca._sixty(rng, 2 * n) for n in (63, 64, 65)]
    buf, offs = sc.pack(wbufs, K16)
    pristine = buf.copy()
    gaps, back = [], []
    for o in offs:
        sca._dead(buf, o[0])
        for i in range(2, len(o), 2):
            flip(buf, o[i], GROW)
            gaps.append(o[i])
            back.append((o[i], sm.sane(pristine, K16, o[i])))
    n = 63 + 64 + 65
    return buf, K16, 4, ON, {"rounds": 1, "headers_repaired": n, "items_repaired": 0, "complete": 1,
                             "first_gaps": gaps, "first_headers": sorted(gaps + [o[0] for o in offs]),
                             "pristine": pristine, "back": back}


def walk_end_is_gap_start():
    """Image 0 (one data bit inverted: a walked kind-0 entry) holds in its value
    the head of a complete stamped image S whose own value ends with image 1,
    byte for byte: the walk passes image 0 and the good image 1 and ends behind
    it, on image 2, whose nkey is 1 -> 0; S, at an uncovered offset, is found
    (kind 4) and ends there too.  The walk end and the gap start are one
    offset, listed once, and image 2's header is repaired once."""
    rng = np.random.default_rng(1309)
    y, z = sc.image_nt(rng, 150), sc.image_nt(rng, 140)
    fill = bytes(rng.integers(0, 256, 40, dtype=np.uint8)) + b"\r\n"
    s_img = sc.stamp(sc.layout.make_item(b"sk", fill + bytes(y[:-2]), cas=None))
    head = bytes(s_img[:len(s_img) - 150])
    x = sc.stamp(sc.layout.make_item(b"xk", bytes(rng.integers(0, 256, 60, dtype=np.uint8)) + head[:-2], cas=None))
    buf, offs = sc.pack([[x, y, z] + sca._imgs(rng, [200])], K2)
    pristine, o = buf.copy(), offs[0]
    at = 48 + 2 + 1 + 60  # S in image 0
    assert bytes(buf[at:at + len(s_img)]) == bytes(s_img) and at + len(s_img) == o[2] and buf[o[2] + 41] == 1
    flip(buf, o[0], sca.DATA)
    flip(buf, o[2], 328)
    return buf, K2, 4, ON, {"complete": 1, "headers_repaired": 1, "items_repaired": 1, "first_gaps": [o[2], o[3] + 200],
                            "first_headers": [0, o[2], o[3] + 200], "first_kinds": {0: 0, at: 4, o[1]: 1},
                            "final": {o[0]: 1, o[2]: 1, o[3]: 1}, "absent": [at], "pristine": pristine,
                            "back": [(o[0], len(x)), (o[2], 140)]}


CASES = {
    "behind": behind, "behind_off": lambda: behind(gaps=False), "neighbour_of_dead": neighbour_of_dead,
    "chain": chain, "chain_two_rounds": lambda: chain(2), "edge": edge, "abutting": abutting,
    "entry_inside": entry_inside, "overlap": overlap, "rounds_of_64": rounds_of_64,
    "cflags64": lambda: behind(cfl=8), "walk_end_is_gap_start": walk_end_is_gap_start,
}
_BUILT = {}


def case(name):
    """The case, built once."""
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]


def check_notes(m, first, notes, kinds0=None):
    """scrub_cases.check_notes and this file's own keys: m the scrub's result
    dict, first = (header list, item list, suspects, gap starts) of the damaged
    page's first triage, kinds0 that triage's offset -> kind."""
    sca.check_notes(m, first[:3], notes)
    if "first_gaps" in notes:
        assert first[3] == notes["first_gaps"], first[3]
    if "first_items" in notes:
        assert first[1] == notes["first_items"], first[1]
    for o, k in notes.get("first_kinds", {}).items():
        assert kinds0[o] == k, (o, kinds0.get(o))
    kinds = dict(zip(m["offsets"], m["kind"]))
    for o, nt in notes["back"]:
        assert kinds.get(o) in (1, 4), (o, kinds.get(o))
        assert (m["after"][o + 28:o + nt] == notes["pristine"][o + 28:o + nt]).all(), o
