"""Buffers for the crc32c_triage_pages tests (the CPU model tests and the GPU
tests share them).  W = 64 KiB, one to three wbufs, images of 60 to 4200 bytes;
each case comes with what it is built to show:

    name -> (buf, W, cfl, notes), notes a dict of offset lists:
      "suspects"    the suspects the case places (any other lies inside one of them)
      "absent"      offsets that no list may name
      "kind0_once"  walked entries with verdict 0 that are failing candidates
      "found"       offsets the salvage must find (kind 4)
      "single_bit"  suspects with one bit inverted (crc32c_repair_items repairs them)
      "two_bit"     suspects with two (it does not)
"""
import struct

import numpy as np

from tests import recover_model as rm
from tests import salvage_cases as sc
from tests import salvage_model as sm

K64 = sc.K64


def _flip(buf, at, mask=0x20):
    buf[at] ^= mask


def _images(rng, nts):
    """Images without CAS: the key at 48, the value from 48 + nkey + 1 to nt - 2."""
    return [sc.image_nt(rng, nt) for nt in nts]


def behind_nkey0():
    """Image 2's nkey is zeroed: the walk of wbuf 1 ends there and the image
    cannot be repaired.  Behind it one bit is inverted in a data byte of image
    4, a key byte of image 6, the stored CRC of image 8, nbytes of image 10 and
    the final LF of image 12; image 14 has two data bits inverted.  The images
    between them are intact."""
    rng = np.random.default_rng(810)
    nts = [300, 700, 1200, 900, 4200, 500, 640, 333, 1500, 60, 2000, 777, 1100, 450, 3000, 250]
    buf, offs = sc.pack([sc.mixed(rng, K64, 0.3), _images(rng, nts)], K64)
    o = offs[1]
    sc.HEADER_DAMAGE["nkey0"](buf, o[2])
    _flip(buf, o[4] + 3000)         # data
    _flip(buf, o[6] + 48, 0x40)     # key
    _flip(buf, o[8] + 29, 0x04)     # stored CRC
    _flip(buf, o[10] + 32, 0x10)    # nbytes
    _flip(buf, o[12] + 1100 - 1, 0x01)  # the LF
    _flip(buf, o[14] + 100)
    _flip(buf, o[14] + 2900, 0x01)
    return buf, K64, 4, {"suspects": [o[4], o[6], o[8], o[14]], "absent": [o[2], o[10], o[12]],
                         "found": [o[k] for k in (3, 5, 7, 9, 11, 13, 15)],
                         "single_bit": [o[4], o[6], o[8]], "two_bit": [o[14]]}


def walked_bad_is_not_listed_twice():
    """A data bit inverted in image 3, which the walk reaches and passes: a
    failing candidate outside the covered set that is a walked entry.  (Image 9's
    zeroed nkey gives the call something to find as well.)"""
    rng = np.random.default_rng(820)
    nts = [400, 90, 1300, 2100, 640, 4000, 75, 800, 512, 1000, 300, 3333, 61]
    buf, offs = sc.pack([_images(rng, nts)], K64)
    o = offs[0]
    _flip(buf, o[3] + 1000)
    sc.HEADER_DAMAGE["nkey0"](buf, o[9])
    return buf, K64, 4, {"suspects": [], "kind0_once": [o[3]], "absent": [o[9]], "found": o[10:]}


def _lookalike(rng, nt):
    """A complete image with a sane header and CRLF whose stored CRC is wrong."""
    img = sc.image_nt(rng, nt)
    img[nt - 20] ^= 0x08
    return img


def suspect_inside_found():
    """An intact image whose value embeds a complete failing look-alike, behind
    a zeroed nkey: the cursor passes over the look-alike with the image found."""
    rng = np.random.default_rng(830)
    value = bytes(rng.integers(0, 256, 200, dtype=np.uint8)) + bytes(_lookalike(rng, 800)) + bytes(
        rng.integers(0, 256, 150, dtype=np.uint8))
    outer = sc.stamp(sc.layout.make_item(b"outer-key", value, cas=None))
    imgs = _images(rng, [500, 1200, 333]) + [outer] + _images(rng, [700, 60])
    buf, offs = sc.pack([sc.mixed(rng, K64, 0.2), imgs, sc.mixed(rng, K64, 0.2)], K64)
    o = offs[1]
    sc.HEADER_DAMAGE["nkey0"](buf, o[1])
    inner = o[3] + 48 + len(b"outer-key") + 1 + 200
    assert sm.candidate(buf, K64, inner) == 800 and not sm.intact(buf, K64, inner)
    return buf, K64, 4, {"suspects": [], "absent": [o[1], inner], "found": o[2:]}


def found_inside_suspect():
    """The damaged image (nkey zeroed) holds a look-alike header in its own value
    bytes whose nbytes makes it end on the CRLF of the second real image behind
    it: a suspect that spans found images."""
    rng = np.random.default_rng(840)
    imgs = _images(rng, [640, 4000, 900, 1500, 350])
    buf, offs = sc.pack([imgs], K64)
    o = offs[0]
    p = o[1] + 1000  # inside image 1's value
    end = o[3] + 1500
    struct.pack_into("<I", buf, p + 32, end - p - 50)  # 48 + nkey 1 + 1 + nbytes = end - p
    buf[p + 38:p + 40] = 0
    buf[p + 41] = 1
    sc.HEADER_DAMAGE["nkey0"](buf, o[1])
    assert sm.candidate(buf, K64, p) == end - p and not sm.intact(buf, K64, p)
    return buf, K64, 4, {"suspects": [p], "absent": [o[1]], "found": o[2:]}


def many_rounds():
    """recover_model.many_found()'s 270 small images with a data bit inverted in
    every 7th: more than four rounds of 64 candidates in one piece, suspects and
    found images alternating across the round boundaries.  (Image 0 is reached
    by the walk: kind 0, no suspect.)"""
    buf, W, cfl = rm.many_found()
    buf = buf.copy()
    o = W
    for _ in range(2):
        o += sm.ntotal_at(buf, o)[0]
    pristine = buf.copy()
    sc.HEADER_DAMAGE["nbytes_b0"](pristine, o)  # (the damage is its own inverse)
    walked, _ = sc.walk_lists(pristine, W, cfl)
    imgs = [x for x in walked.tolist() if W <= x < 2 * W]
    assert len(imgs) == 270 and imgs[2] == o
    hit = imgs[0::7]
    for at in hit:
        _flip(buf, at + sm.ntotal_at(buf, at)[0] - 3, 0x02)  # the value's last byte
    return buf, W, cfl, {"suspects": hit[1:], "kind0_once": hit[:1], "single_bit": hit[1:],
                         "found": [x for k, x in enumerate(imgs) if k > 2 and k % 7]}


def work_bound():
    buf, W = rm.work_bound_behind_a_walk()
    return buf, W, 4, {"suspects": []}


def built():
    """The cases built for the suspects."""
    return {f.__name__: f() for f in (behind_nkey0, walked_bad_is_not_listed_twice, suspect_inside_found,
                                      found_inside_suspect, many_rounds, work_bound)}


def reused():
    """The salvage's own small buffers, unchanged: most have no suspect."""
    out = {name: case + ({},) for name, case in sc.small_cases().items()}
    out["hand_built"] = sc.hand_built() + (4, {})
    return out


def config5():
    return sc.config5_case(8) + (4, {"suspects": []})


def check_notes(m, notes):
    """A case's own assertions on a result dict (the model's, or the library's
    in the same shape): offsets, kind."""
    kinds = {}
    for o, k in zip(m["offsets"], m["kind"]):
        kinds.setdefault(o, []).append(k)
    suspects = [o for o, k in zip(m["offsets"], m["kind"]) if k == 6]
    assert suspects == sorted(suspects)
    if "suspects" in notes:
        # every one named is listed; any other lies inside a named one's own unproven bytes (an image of under
        # 570 bytes without CAS reads as a second header 9 bytes in -- nbytes' = its nkey, nkey' = its third
        # key byte -- that ends on its CRLF once in 256: many_rounds has one)
        assert set(notes["suspects"]) <= set(suspects)
        spans = [(o, o + m["lens"][m["offsets"].index(o)]) for o in notes["suspects"]]
        for o in set(suspects) - set(notes["suspects"]):
            assert any(lo < o < hi for lo, hi in spans), o
    for o in notes.get("absent", ()):
        assert o not in kinds, o
    for o in notes.get("kind0_once", ()):
        assert kinds[o] == [0], o
    for o in notes.get("found", ()):
        assert kinds[o] == [4], o
    assert all(len(v) == 1 for v in kinds.values())  # no offset twice
    assert m["nsuspect"] == len(suspects) <= m["ncand"] - m["nsalvaged"]
