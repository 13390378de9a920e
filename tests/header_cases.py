"""Buffers for the crc32c_repair_headers tests (no GPU, no library call): the
CPU model tests and the GPU tests share them."""
import numpy as np

from tests import header_model as hm
from tests import oracle
from tests import salvage_cases as sc
from tests import salvage_model as sm
from tests.repair_cases import flip, place


def per_region(img, bits, region=128, aligns=16):
    """One copy of img per region and (alignment, bit), that bit inverted:
    (buffer, offsets, bits, the buffer with every copy pristine)."""
    nt = len(img)
    assert nt + aligns <= region
    buf = np.zeros(aligns * len(bits) * region, np.uint8)
    offs, flipped = [], []
    for a in range(aligns):
        for j, k in enumerate(bits):
            o = (a * len(bits) + j) * region + a
            buf[o:o + nt] = np.frombuffer(bytes(img), np.uint8)
            offs.append(o)
            flipped.append(k)
    pristine = buf.copy()
    for o, k in zip(offs, flipped):
        flip(buf, o, k)
    return buf, np.array(offs, np.uint64), flipped, pristine


def packed(rng, cfl=4):
    """Images of nt = 52..80 and 4164..4166, each with each of the 42 bits
    inverted and once intact, packed with lead 3 and no region:
    (buffer, offsets, bits (None: intact), ntotals)."""
    images, bits = [], []
    for i, nt in enumerate(list(range(52, 81)) + [4164, 4165, 4166]):
        cas = bool(i & 1) and nt >= 61 + cfl
        cflags = 0x01020304 if i % 3 == 0 and nt >= 61 + cfl else 0
        img = sc.image_nt(rng, nt, cas=cas, cflags=cflags, cfl=cfl)
        for k in hm.BITS + [None]:
            images.append(img)
            bits.append(k)
    buf, offs = place(images, align=1, lead=3)
    for o, k in zip(offs.tolist(), bits):
        if k is not None:
            flip(buf, o, k)
    return buf, offs, bits, [len(img) for img in images]


def _solve4(buf, at, lo, hi, want):
    """Set the four bytes at ``at`` so that crc32c(0, buf[lo:hi]) == want (the
    CRC is affine in them and 32 consecutive bits map onto it one to one)."""
    buf[at:at + 4] = 0
    c0 = oracle.crc32c(0, buf[lo:hi])
    rows = []  # (the CRC's change, the bit of the four bytes that makes it)
    for i in range(32):
        buf[at + i // 8] ^= 1 << (i % 8)
        rows.append([oracle.crc32c(0, buf[lo:hi]) ^ c0, 1 << i])
        buf[at + i // 8] ^= 1 << (i % 8)
    need, x = c0 ^ want, 0
    for b in range(32):  # Gauss-Jordan over GF(2): row b ends as the one with CRC bit b alone
        p = next(r for r in range(b, 32) if rows[r][0] >> b & 1)
        rows[b], rows[p] = rows[p], rows[b]
        for r in range(32):
            if r != b and rows[r][0] >> b & 1:
                rows[r][0] ^= rows[b][0]
                rows[r][1] ^= rows[b][1]
    for b in range(32):
        if need >> b & 1:
            x ^= rows[b][1]
    buf[at:at + 4] = np.frombuffer(int(x).to_bytes(4, "little"), np.uint8)
    assert oracle.crc32c(0, buf[lo:hi]) == want


def ambiguous(crafted=True):
    """An intact 77-byte image at offset 5 with nbytes bit 0 inverted; with
    ``crafted`` four bytes in front of a CRLF at the end of the variant with
    nbytes bit 5 are solved so that its CRC hits too.  (buffer, offset)."""
    rng = np.random.default_rng(77)
    o, k2 = 5, 256 + 5
    buf = np.zeros(256, np.uint8)
    buf[o + 77:] = rng.integers(1, 256, 256 - o - 77, dtype=np.uint8)
    buf[o:o + 77] = np.frombuffer(bytes(sc.image_nt(rng, 77)), np.uint8)
    flip(buf, o, 256)
    if crafted:
        flip(buf, o, k2)
        nt2 = sm.sane(buf, 1 << 62, o)
        assert nt2 > 77 + 6 and o + nt2 <= buf.size
        buf[o + nt2 - 2:o + nt2] = (13, 10)
        # (with bit k2 inverted, as the rule computes that variant's CRC)
        _solve4(buf, o + nt2 - 6, o + 32, o + nt2, int.from_bytes(bytes(buf[o + 28:o + 32]), "little"))
        flip(buf, o, k2)
    return buf, o


def mixed_damage():
    """(buffer, offsets, names): one image per kind of damage the call must
    leave alone, and decoys that must change no verdict."""
    rng = np.random.default_rng(42)
    names = ["data_bit", "two_length_bits", "length_and_data", "nkey0", "no_crlf", "decoy", "intact", "one_bit"]
    images = [sc.image_nt(rng, 300 + 7 * i, cas=bool(i & 1)) for i in range(len(names))]
    images[names.index("nkey0")] = sc.image_nt(rng, 303)  # (nt % 7 == 2: nkey 3)
    images[names.index("no_crlf")] = sc.raw_image(rng, 300, b"xy")
    buf, offs = place(images, align=512, lead=9)
    at = dict(zip(names, offs.tolist()))
    flip(buf, at["data_bit"], 8 * 100 + 3)
    flip(buf, at["two_length_bits"], 256 + 2)
    flip(buf, at["two_length_bits"], 256 + 4)
    flip(buf, at["length_and_data"], 256 + 3)
    flip(buf, at["length_and_data"], 8 * 90)
    assert buf[at["nkey0"] + 41] == 3
    buf[at["nkey0"] + 41] = 0
    flip(buf, at["no_crlf"], 256 + 1)
    # one bit, with a CRLF planted where a wrong variant (nbytes bit 6 on top of the damage) would end
    for name in ("decoy", "one_bit"):
        flip(buf, at[name], 256 + 3)
    o, true_nt = at["decoy"], len(images[names.index("decoy")])
    for b in (6, 5, 7):  # (the first that lengthens the image: the CRLF lands behind it)
        flip(buf, o, 256 + b)
        nt = sm.sane(buf, 1 << 62, o)
        flip(buf, o, 256 + b)
        if nt >= true_nt + 2:
            break
    assert nt >= true_nt + 2 and o + nt < at["intact"]
    buf[o + nt - 2:o + nt] = (13, 10)
    return buf, offs, names


def breaks_from(offs, lens, kind, nbytes, W):
    """The list for crc32c_repair_headers from crc32c_recover_pages' three
    arrays (or the walk's lists with ITEM_ntotals): every kind 0 entry, and each
    piece's walk end when it is not itself an entry -- the end of the piece's
    last walked entry when that is good, the piece's start when it has none --
    when at least 48 bytes of the piece remain there."""
    offs, lens, kind = (np.asarray(x).tolist() for x in (offs, lens, kind))
    out = [o for o, k in zip(offs, kind) if k == 0]
    last = {}  # piece -> its last walked entry
    for o, n, k in zip(offs, lens, kind):
        if k in (0, 1):
            last[o // W] = (o, n, k)
    for w in range(-(-nbytes // W)):
        pe = min((w + 1) * W, nbytes)
        if w not in last:
            end = w * W
        elif last[w][2] == 1:
            end = last[w][0] + last[w][1]
        else:
            continue
        if pe - end >= 48:
            out.append(end)
    return np.array(sorted(set(out)), np.uint64)


def breaks(buf, W, cfl=4):
    """breaks_from over the walk's own lists (tests/salvage_cases.walk_lists)."""
    buf = sm._u8(buf)
    offs, ok = sc.walk_lists(buf, W, cfl)
    lens = [sm.sane(buf, W, int(o), cfl) for o in offs.tolist()]
    return breaks_from(offs, lens, ok, len(buf), W)
