"""Pages for the crc32c_scrub_pages tests (no GPU, no library call): the CPU
model tests and the GPU tests share them.  Pieces of 2 to 8 KiB, images of 60
to 600 bytes, at most 8 pieces; each case is the smallest page at which one
step of the flow can go wrong.

    name -> (buf, W, cfl, kwargs of the call, notes)

notes: what the case is built to show, checked on the model's result by
``check_notes`` (and so, through the exact comparison, on the library's)."""
import struct

import numpy as np

from tests import salvage_cases as sc
from tests import salvage_model as sm
from tests import triage_cases as tc
from tests.repair_cases import flip

K2, K4, K8 = 2 << 10, 4 << 10, 8 << 10
GROW = 256 + 20  # nbytes bit 20: the image would end a MiB on, past any piece here
DATA = 8 * 50 + 3  # a bit of byte 50: key or value of every image here


def _imgs(rng, nts, cfl=4, cflags_every=0):
    return [sc.image_nt(rng, nt, cflags=0x01020304 if cflags_every and i % cflags_every == 0 else 0, cfl=cfl)
            for i, nt in enumerate(nts)]


def _dead(buf, o):
    """nkey 3 -> 0: two bits, no rule fixes it, and the walk ends there."""
    assert buf[o + 41] == 3
    buf[o + 41] = 0


def clean():
    rng = np.random.default_rng(1201)
    buf, _ = sc.pack([_imgs(rng, [60, 333, 600, 128]), _imgs(rng, [250, 90]), _imgs(rng, [599, 61, 61])], K2)
    return buf, K2, 4, {}, {"rounds": 0, "nflips": 0, "complete": 1}


def two_rounds():
    """Images 1 and 2 of piece 0 each with nbytes bit 20 inverted: the walk ends
    at image 1 and image 2 is no candidate, so it is reached only once image 1
    is repaired."""
    rng = np.random.default_rng(1202)
    buf, offs = sc.pack([_imgs(rng, [200, 300, 150, 400, 90]), _imgs(rng, [500, 77])], K2)
    o = offs[0]
    flip(buf, o[1], GROW)
    flip(buf, o[2], GROW)
    return buf, K2, 4, {}, {"rounds": 2, "headers_repaired": 2, "items_repaired": 0, "complete": 1,
                            "log": [(o[1], GROW, 1), (o[2], GROW, 1)], "final": {o[1]: 1, o[2]: 1, o[3]: 1}}


def two_rounds_one_allowed():
    buf, W, cfl, _, _ = two_rounds()
    return buf, W, cfl, {"max_rounds": 1}, {"rounds": 1, "headers_repaired": 1, "complete": 0, "rc": 0}


def suspect_promotion(cfl=4):
    """Image 1's nkey zeroed, image 3 behind it with one data bit inverted: a
    suspect, then repaired, then found (kind 4); image 1 stays lost."""
    rng = np.random.default_rng(1203)
    buf, offs = sc.pack([_imgs(rng, [300, 359, 222, 500, 140], cfl, 2), _imgs(rng, [100, 200], cfl, 2)], K2)
    o = offs[0]
    _dead(buf, o[1])
    flip(buf, o[3], DATA + 8 * 100)
    return buf, K2, cfl, {}, {"rounds": 1, "headers_repaired": 0, "items_repaired": 1, "complete": 1,
                              "log": [(o[3], DATA + 8 * 100, 2)], "final": {o[3]: 4, o[2]: 4, o[4]: 4},
                              "absent": [o[1]]}


def suspect_promotion_cflags64():
    return suspect_promotion(8)


def kind0_entry():
    rng = np.random.default_rng(1204)
    buf, offs = sc.pack([_imgs(rng, [120, 480, 333])], K2)
    o = offs[0]
    flip(buf, o[1], DATA)
    return buf, K2, 4, {}, {"rounds": 1, "items_repaired": 1, "complete": 1, "log": [(o[1], DATA, 2)],
                            "final": {o[1]: 1}}


def two_bits():
    rng = np.random.default_rng(1205)
    buf, offs = sc.pack([_imgs(rng, [120, 480, 333])], K2)
    o = offs[0]
    flip(buf, o[1], DATA)
    flip(buf, o[1], DATA + 8 * 200 + 1)
    return buf, K2, 4, {}, {"rounds": 0, "nflips": 0, "complete": 1, "final": {o[1]: 0}}


def dropped_lookalike():
    """triage_cases.found_inside_suspect's look-alike at this size -- a header in
    the dead image 1's value whose length ends on image 3's CRLF: a suspect
    that spans found images -- and image 4, one data bit inverted, whose value
    holds a complete failing look-alike: two overlapping suspects."""
    rng = np.random.default_rng(1206)
    inner = tc._lookalike(rng, 200)
    value = bytes(rng.integers(0, 256, 50, dtype=np.uint8)) + bytes(inner) + bytes(
        rng.integers(0, 256, 60, dtype=np.uint8))
    outer = sc.stamp(sc.layout.make_item(b"xk", value, cas=None))
    imgs = _imgs(rng, [200, 597, 300, 400]) + [outer] + _imgs(rng, [150])
    buf, offs = sc.pack([imgs], K4)
    o = offs[0]
    p, end = o[1] + 150, o[3] + 400
    struct.pack_into("<I", buf, p + 32, end - p - 50)  # 48 + nkey 1 + 1 + nbytes = end - p
    buf[p + 38:p + 40] = 0
    buf[p + 41] = 1
    _dead(buf, o[1])
    y = o[4] + 48 + 2 + 1 + 50
    k = 8 * (48 + 2 + 1 + 10)  # in the outer value, in front of the look-alike
    flip(buf, o[4], k)
    assert sm.candidate(buf, K4, p) == end - p and not sm.intact(buf, K4, p)
    assert sm.candidate(buf, K4, y) == 200 and not sm.intact(buf, K4, y)
    return buf, K4, 4, {}, {"rounds": 1, "items_repaired": 1, "complete": 1, "log": [(o[4], k, 2)],
                            "first_suspects": [p, o[4], y], "first_kept": [o[4]],
                            "final": {p: 6, o[2]: 4, o[3]: 4, o[4]: 4, o[5]: 4}, "absent": [y, o[1]]}


def second_pass():
    """Piece 0's image 2 is sane with one data bit inverted and image 3's nkey
    is 1 -> 0, a length bit: the walk ends at image 3 with a kind-0 entry last,
    so the walk end is listed only once the item repair has made image 2 good.
    The documents' written-out flow (headers, then items, once) leaves image 3."""
    rng = np.random.default_rng(1207)
    buf, offs = sc.pack([_imgs(rng, [100, 250, 330, 70 * 7, 160]), _imgs(rng, [90])], K2)
    o = offs[0]
    flip(buf, o[2], DATA)
    assert buf[o[3] + 41] == 1
    flip(buf, o[3], 328)
    return buf, K2, 4, {}, {"rounds": 2, "headers_repaired": 1, "items_repaired": 1, "complete": 1,
                            "log": [(o[2], DATA, 2), (o[3], 328, 1)], "final": {o[2]: 1, o[3]: 1, o[4]: 1},
                            "single_pass_leaves": [o[3]]}


def work_bound():
    buf, W, cfl, _ = tc.work_bound()
    return buf, W, cfl, {}, {"rc": -7, "nflips": 0, "rounds": 0, "complete": 0}


def geometry():
    """Piece 0 filled to 47 bytes before its end, piece 1 to 48, piece 2 empty,
    piece 3 cut short by the page's end."""
    rng = np.random.default_rng(1210)
    a = _imgs(rng, [600, 600, 600, K2 - 47 - 1800])
    b = _imgs(rng, [500, 500, 500, K2 - 48 - 1500])
    buf, offs = sc.pack([a, b, [], _imgs(rng, [300, 200])], K2, total=3 * K2 + 700)
    return buf, K2, 4, {}, {"rounds": 0, "complete": 1,
                            "first_headers": [2 * K2 - 48, 2 * K2, 3 * K2 + 500]}


def _sixty(rng, n):
    return _imgs(rng, [60 + (i % 5) for i in range(n)])


def suspects_per_piece():
    """Pieces with 63, 64 and 65 damaged images behind a dead first one: as
    many suspects (and kept ones) a piece, around k_scrub_items' round of 64."""
    rng = np.random.default_rng(1214)
    wbufs, want = [], []
    for n in (63, 64, 65):
        wbufs.append(_imgs(rng, [72]) + _sixty(rng, n))
    buf, offs = sc.pack(wbufs, K8)
    for o in offs:
        _dead(buf, o[0])
        for at in o[1:]:
            flip(buf, at, DATA)
        want += o[1:]
    return buf, K8, 4, {}, {"rounds": 1, "items_repaired": 63 + 64 + 65, "complete": 1, "first_kept": want}


def entries_per_piece():
    """Pieces of 63, 64 and 65 walked images, every one with a data bit
    inverted: kind-0 entries around both list kernels' round of 64."""
    rng = np.random.default_rng(1215)
    buf, offs = sc.pack([_sixty(rng, n) for n in (63, 64, 65)], K8)
    for o in offs:
        for at in o:
            flip(buf, at, DATA)
    return buf, K8, 4, {}, {"rounds": 1, "items_repaired": 63 + 64 + 65, "complete": 1,
                            "first_headers_n": 63 + 64 + 65}


def log_round(n):
    """n walked images in 8 pieces, every one with a data bit inverted: a repair
    list and a log of n entries, around k_scrub_log's round of 1024."""
    rng = np.random.default_rng(1216)
    per = [n // 8 + (1 if w < n % 8 else 0) for w in range(8)]
    buf, offs = sc.pack([_sixty(rng, m) for m in per], K8)
    for o in offs:
        for at in o:
            flip(buf, at, DATA)
    return buf, K8, 4, {}, {"rounds": 1, "items_repaired": n, "nflips": n, "complete": 1}


CASES = {
    "clean": clean, "two_rounds": two_rounds, "suspect_promotion": suspect_promotion, "kind0_entry": kind0_entry,
    "two_bits": two_bits, "dropped_lookalike": dropped_lookalike, "second_pass": second_pass,
    "two_rounds_one_allowed": two_rounds_one_allowed, "work_bound": work_bound, "geometry": geometry,
    "suspect_promotion_cflags64": suspect_promotion_cflags64, "suspects_per_piece": suspects_per_piece,
    "entries_per_piece": entries_per_piece, "log_1023": lambda: log_round(1023), "log_1024": lambda: log_round(1024),
    "log_1025": lambda: log_round(1025),
}
_BUILT = {}


def case(name):
    """The case, built once."""
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]


def check_notes(m, first, notes):
    """A case's own assertions: m the scrub's result dict, first = (header
    list, item list, suspects) of the damaged page's first triage."""
    for key in ("rc", "rounds", "nflips", "headers_repaired", "items_repaired", "complete"):
        if key in notes:
            assert m[key] == notes[key], (key, m[key])
    if "log" in notes:
        assert list(zip(m["flip_offsets"], m["flip_bits"], m["flip_by"])) == notes["log"]
    kinds = dict(zip(m["offsets"], m["kind"]))
    for o, k in notes.get("final", {}).items():
        assert kinds.get(o) == k, (o, kinds.get(o))
    for o in notes.get("absent", ()):
        assert o not in kinds, o
    headers, items, suspects = first
    if "first_headers" in notes:
        assert headers == notes["first_headers"]
    if "first_headers_n" in notes:
        assert len(headers) == notes["first_headers_n"]
    if "first_suspects" in notes:
        assert suspects == notes["first_suspects"]
    if "first_kept" in notes:
        assert [o for o in items if o in set(suspects)] == notes["first_kept"]
