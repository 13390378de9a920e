"""Buffers for the crc32c_salvage_pages tests (CPU model tests and GPU tests
share them): wbufs of stamped item images with one kind of damage each."""
import struct

import numpy as np

from memcached_amd import layout
from tests import oracle

K16, K64 = 16 << 10, 64 << 10


def stamp(img):
    img[28:32] = struct.pack("<I", oracle.crc32c(0, bytes(img[32:])))
    return img


def image_nt(rng, nt, cas=False, cflags=0, cfl=4, value=None):
    """A stamped image of exactly nt bytes (random key without NULs, random value + CRLF)."""
    fixed = 48 + 1 + 2 + (8 if cas else 0) + (cfl if cflags else 0)
    nkey = min(1 + nt % 7, nt - fixed)
    assert nkey >= 1, nt
    key = bytes(rng.integers(1, 256, nkey, dtype=np.uint8))
    if value is None:
        value = bytes(rng.integers(0, 256, nt - fixed - nkey, dtype=np.uint8))
    img = layout.make_item(key, value, cas=7 if cas else None, client_flags=cflags, cflags_bytes=cfl)
    assert len(img) == nt, (len(img), nt)
    return stamp(img)


def raw_image(rng, nbytes, tail):
    """A stamped image whose nbytes field and last bytes are set freely (no CAS, 3-byte key)."""
    img = bytearray(48 + 4 + nbytes)
    struct.pack_into("<IIiHHBB", img, 24, 0, 0, nbytes, 1, 0, 1, 3)
    img[48:51] = b"key"
    img[52:] = bytes(rng.integers(0, 256, nbytes, dtype=np.uint8))
    if tail:
        img[len(img) - len(tail):] = tail
    return stamp(img)


def pack(wbufs, W, total=None):
    """wbufs: a list of image lists, each packed from its wbuf's first byte.
    Returns (buffer, per-wbuf lists of image offsets)."""
    buf = np.zeros(len(wbufs) * W, np.uint8)
    offs = []
    for w, imgs in enumerate(wbufs):
        o, mine = w * W, []
        for img in imgs:
            assert o + len(img) <= (w + 1) * W
            buf[o:o + len(img)] = np.frombuffer(bytes(img), np.uint8)
            mine.append(o)
            o += len(img)
        offs.append(mine)
    return (buf if total is None else buf[:total].copy()), offs


def mixed(rng, W, fill=0.8):
    """Images of mixed sizes filling about `fill` of a wbuf."""
    imgs, used = [], 0
    while True:
        nt = int(rng.integers(60, 1500))
        if used + nt > W * fill:
            return imgs
        imgs.append(image_nt(rng, nt, cas=bool(nt & 1)))
        used += nt


HEADER_DAMAGE = {
    "nkey0": lambda b, o: b.__setitem__(o + 41, 0),
    "nbytes_b0": lambda b, o: b.__setitem__(o + 32, b[o + 32] ^ 0x10),
    "nbytes_b1": lambda b, o: b.__setitem__(o + 33, b[o + 33] ^ 0x02),
    "nbytes_b2": lambda b, o: b.__setitem__(o + 34, b[o + 34] ^ 0x01),
    "nbytes_b3": lambda b, o: b.__setitem__(o + 35, b[o + 35] ^ 0x80),
    "cas_bit": lambda b, o: b.__setitem__(o + 38, b[o + 38] ^ 0x02),
    "cflags_bit": lambda b, o: b.__setitem__(o + 39, b[o + 39] ^ 0x01),
    "nkey_other": lambda b, o: b.__setitem__(o + 41, b[o + 41] ^ 0x04),
}


def data_damage(b, o):
    b[o + 57] ^= 0x20


def walk_lists(buf, W, cfl=4):
    """What crc32c_verify_pages returns: the sequential walk of every piece
    (storage.c:950-1070) and, per image, sane and stored CRC matching."""
    from tests import salvage_model as sm
    n, offs, ok = len(buf), [], []
    for ps in range(0, n, W):
        pe, o = min(ps + W, n), ps
        while o + 48 <= pe and buf[o + 41] != 0:
            nt = sm.sane(buf, W, o, cfl)
            good = bool(nt) and oracle.crc32c(0, buf[o + 32:o + nt]) == int.from_bytes(bytes(buf[o + 28:o + 32]),
                                                                                        "little")
            offs.append(o)
            ok.append(1 if good else 0)
            o += sm.ntotal_at(buf, o, cfl)[0]
    return np.array(offs, np.uint64), np.array(ok, np.uint8)


def hand_built():
    """One wbuf of five 1000-byte images, image 2's nkey zeroed."""
    rng = np.random.default_rng(11)
    buf, offs = pack([[image_nt(rng, 1000) for _ in range(5)]], K16)
    buf[2000 + 41] = 0
    return buf, K16


# the cases of small_cases() that the GPU tests of every page-recovery call run by name
SMALL = ["hdr_" + k for k in HEADER_DAMAGE] + [
    "data_only", "first_image", "last_image", "two_adjacent", "header_then_data", "ends_exact", "ends_one_short",
    "lookalike_in_intact", "lookalike_in_damaged", "no_crlf", "cflags64", "cflags64_read_as_32", "config5_small",
    "ranges_6", "ranges_over_64"]


def small_cases():
    """name -> (buf, W, cfl): every case small enough for the byte-by-byte model."""
    out = {}
    for i, (name, hit) in enumerate(HEADER_DAMAGE.items()):
        rng = np.random.default_rng(100 + i)
        buf, offs = pack([mixed(rng, K16) for _ in range(3)], K16)
        hit(buf, offs[1][len(offs[1]) // 2])
        out["hdr_" + name] = (buf, K16, 4)
    rng = np.random.default_rng(200)
    buf, offs = pack([mixed(rng, K16) for _ in range(3)], K16)
    data_damage(buf, offs[0][3])
    data_damage(buf, offs[2][1])
    out["data_only"] = (buf, K16, 4)

    buf, offs = pack([mixed(rng, K16) for _ in range(3)], K16)
    HEADER_DAMAGE["nkey0"](buf, offs[1][0])
    HEADER_DAMAGE["nbytes_b1"](buf, offs[2][0])
    out["first_image"] = (buf, K16, 4)

    buf, offs = pack([mixed(rng, K16) for _ in range(3)], K16)
    HEADER_DAMAGE["nkey0"](buf, offs[1][-1])
    out["last_image"] = (buf, K16, 4)

    buf, offs = pack([mixed(rng, K16) for _ in range(3)], K16)
    HEADER_DAMAGE["nkey0"](buf, offs[1][4])
    HEADER_DAMAGE["nbytes_b0"](buf, offs[1][5])
    out["two_adjacent"] = (buf, K16, 4)

    buf, offs = pack([mixed(rng, K16) for _ in range(3)], K16)
    HEADER_DAMAGE["cas_bit"](buf, offs[1][2])
    data_damage(buf, offs[1][3])
    out["header_then_data"] = (buf, K16, 4)

    # ends: wbuf 0 full to its last byte behind a damaged image, wbuf 1's
    # last image a 52-byte one ending at the piece end (its header in the
    # last 52 bytes), an open last piece ending with its last image -- and the
    # same buffer one byte shorter, where that image no longer fits
    def full(nts, W=K16):
        imgs = [image_nt(rng, nt) for nt in nts]
        used = sum(nts)
        return imgs + [image_nt(rng, W - used)] if used < W else imgs
    w0 = full([700, 900, 1300, 5000, 4000, 3000])
    w1 = full([800, 600, K16 - 800 - 600 - 52])
    w2 = [image_nt(rng, nt) for nt in (500, 640, 1111)]
    buf, offs = pack([w0, w1, w2], K16, total=2 * K16 + 500 + 640 + 1111)
    for w in range(3):
        HEADER_DAMAGE["nkey0"](buf, offs[w][1])
    out["ends_exact"] = (buf, K16, 4)
    out["ends_one_short"] = (buf[:-1].copy(), K16, 4)
    out["under_48_bytes"] = (buf[:40].copy(), K16, 4)

    # look-alikes: a complete valid image inside another image's value
    inner = image_nt(rng, 1777)  # (longer than any image of mixed(): told apart by its size)
    value = bytes(rng.integers(0, 256, 300, dtype=np.uint8)) + bytes(inner) + bytes(
        rng.integers(0, 256, 123, dtype=np.uint8))
    for name, damaged in (("lookalike_in_intact", False), ("lookalike_in_damaged", True)):
        outer = stamp(layout.make_item(b"outer-key", value, cas=None))
        imgs = mixed(rng, K16, 0.3) + [outer] + mixed(rng, K16, 0.3)
        buf, offs = pack([mixed(rng, K16), imgs], K16)
        if damaged:
            HEADER_DAMAGE["nkey0"](buf, offs[1][imgs.index(outer)])
        else:
            HEADER_DAMAGE["nkey0"](buf, offs[0][2])
        out[name] = (buf, K16, 4)

    # behind the damage: images without CRLF, with nbytes 0 and 1, then good ones
    imgs = mixed(rng, K16, 0.2) + [raw_image(rng, 300, b"xy"), raw_image(rng, 0, b""), raw_image(rng, 1, b""),
                                   raw_image(rng, 2, b"\r\n"), raw_image(rng, 400, b"\n\r")] + mixed(rng, K16, 0.2)
    buf, offs = pack([imgs], K16)
    HEADER_DAMAGE["nkey0"](buf, offs[0][1])
    out["no_crlf"] = (buf, K16, 4)

    # 8-byte client flags: sane with cfl = 8, and whatever the model says with 4
    imgs = [image_nt(rng, int(rng.integers(80, 900)), cas=bool(k & 1), cflags=0x0123456789 if k % 3 else 0, cfl=8)
            for k in range(24)]
    buf, offs = pack([imgs, list(imgs)], K16)
    HEADER_DAMAGE["nkey0"](buf, offs[0][3])
    HEADER_DAMAGE["cflags_bit"](buf, offs[1][5])
    out["cflags64"] = (buf, K16, 8)
    out["cflags64_read_as_32"] = (buf, K16, 4)

    # more uncovered entries in one piece than the region pass keeps ranges
    # for (4): six data-damaged images in one 16 KiB wbuf, the first a long
    # one whose range spans three 4 KiB tiles
    imgs = [image_nt(rng, 500), image_nt(rng, 9000)] + [image_nt(rng, int(rng.integers(60, 400))) for _ in range(14)]
    buf, offs = pack([mixed(rng, K16), imgs], K16)
    for k in (1, 3, 4, 8, 11, 15):
        data_damage(buf, offs[1][k])
    out["ranges_6"] = (buf, K16, 4)

    # ... and more than a round of 64 entries: a 64 KiB wbuf of some 270 small
    # images with every fourth one data-damaged (65 or so ranges, in every
    # round of the piece's entries), a long damaged image among them, a damaged
    # header near the end, and a clean wbuf on either side
    imgs = [image_nt(rng, int(rng.integers(60, 260)), cas=bool(k & 1)) for k in range(140)]
    imgs += [image_nt(rng, 13000)] + [image_nt(rng, int(rng.integers(60, 260))) for _ in range(130)]
    buf, offs = pack([mixed(rng, K64, 0.2), imgs, mixed(rng, K64, 0.2)], K64)
    assert len(offs[1]) > 4 * 64
    for k in range(2, len(offs[1]), 4):
        data_damage(buf, offs[1][k])
    data_damage(buf, offs[1][140])
    HEADER_DAMAGE["nkey0"](buf, offs[1][255])
    out["ranges_over_64"] = (buf, K64, 4)

    # config 5 in small: 4165-byte images, 64 KiB wbufs
    buf, offs = pack([[image_nt(rng, 4165, cas=True) for _ in range(15)] for _ in range(3)], K64)
    HEADER_DAMAGE["nbytes_b0"](buf, offs[0][2])
    HEADER_DAMAGE["nkey0"](buf, offs[2][7])
    out["config5_small"] = (buf, K64, 4)
    return out


def work_bound_case():
    """W = 64 KiB: a damaged first image whose value holds a fake header every
    64 bytes, all ending at the image's own CRLF."""
    rng = np.random.default_rng(300)
    nt = 60000
    big = image_nt(rng, nt)
    for p in range(128, nt - 200, 64):
        struct.pack_into("<I", big, p + 32, nt - p - 50)  # nbytes: 48 + nkey 1 + 1 + nbytes = nt - p
        big[p + 38:p + 40] = b"\0\0"
        big[p + 41] = 1
    stamp(big)
    buf, offs = pack([[big] + [image_nt(rng, 700) for _ in range(5)]], K64)
    HEADER_DAMAGE["nkey0"](buf, 0)
    return buf, K64


def alignment_case(nwbufs=4200):
    """Wbuf k: a first image of 60 + k bytes with nkey zeroed, a 300-byte and a
    4165-byte image behind it: the survivors' starts cover every residue mod 4096."""
    rng = np.random.default_rng(400)
    a, b = image_nt(rng, 300), image_nt(rng, 4165, cas=True)
    buf = np.zeros(nwbufs * K16, np.uint8)
    tail = np.frombuffer(bytes(a) + bytes(b), np.uint8)
    for k in range(nwbufs):
        first = np.frombuffer(bytes(image_nt(rng, 60 + k)), np.uint8).copy()
        first[41] = 0
        o = k * K16
        buf[o:o + 60 + k] = first
        buf[o + 60 + k:o + 60 + k + tail.size] = tail
    return buf, K16


def config5_case(nwbufs=8):
    """8 wbufs of 4 MiB with 1007 images of 4165 B, one header bit flipped in
    three of them (300 to 1000 survivors behind each)."""
    rng = np.random.default_rng(500)
    W = 4 << 20
    buf = np.zeros(nwbufs * W, np.uint8)
    for w in range(nwbufs):
        body = rng.integers(0, 256, 1007 * 4165, dtype=np.uint8)
        img = np.frombuffer(bytes(image_nt(rng, 4165, cas=True)), np.uint8)
        for i in range(1007):
            o = i * 4165
            body[o:o + 56] = img[:56]
            body[o + 4163:o + 4165] = (13, 10)
        buf[w * W:w * W + body.size] = body
    lens = np.full(nwbufs * 1007, 4165 - 32, np.uint64)
    offs = (np.repeat(np.arange(nwbufs, dtype=np.uint64) * W, 1007) +
            np.tile(np.arange(1007, dtype=np.uint64) * 4165, nwbufs))
    crcs = oracle.batch(buf, offs + 32, lens)
    for o, c in zip(offs.tolist(), crcs.tolist()):
        buf[o + 28:o + 32] = np.frombuffer(struct.pack("<I", c), np.uint8)
    HEADER_DAMAGE["nkey0"](buf, 1 * W + 6 * 4165)
    HEADER_DAMAGE["nbytes_b1"](buf, nwbufs // 2 * W + 400 * 4165)
    HEADER_DAMAGE["cas_bit"](buf, (nwbufs - 1) * W + 700 * 4165)
    return buf, W
