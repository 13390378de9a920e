"""The rule of crc32c_repair_items (include/crc32c_batch.h) restated over
numpy, with the CRCs from the CPU oracle.  Nothing here comes from the library.

The rule is stated twice.  ``located_brute`` is the rule as written: invert each
bit of the stored CRC and the span in turn, recompute the CRC through the
oracle, keep the bits after which stored and computed agree (for short images).
``located_syndrome`` is its syndrome form: S = computed ^ stored, and the bit
with g(t) == S for the sequence g(0) = 0x80000000, g(t + 1) = (g(t) >> 1) ^
(g(t) & 1 ? 0x82F63B78 : 0), found by baby steps and giant steps (for long
ones).  ``repair_one`` is the whole verdict of one image, ``repair`` of a list.

The search's geometry (memcached_amd/csrc/repair_geom.h) is restated too, so
that the tests can put damage on both sides of its boundaries."""
import numpy as np

from tests import oracle
from tests import salvage_model as sm

POLY = 0x82F63B78
ONE = 0x80000000
ORDER = (1 << 31) - 1  # of x mod P
NO_BIT = (1 << 64) - 1
REPAIRED = 5
SPAN_DEFAULT = 2 << 20
SPAN_MAX = 0x0FFFFFC0
CHUNK = 256  # byte steps (8 positions each) a lane of the search takes


def step(g):
    return (g >> 1) ^ (POLY if g & 1 else 0)


def mulmod(a, b):
    """a b mod P, both reflected (bit 31 = x^0)."""
    prod = 0
    for i in range(31, -1, -1):
        if (a >> i) & 1:
            prod ^= b
        b = step(b)
    return prod


def xpow(t):
    """g(t) = x^t mod P."""
    r, base = ONE, ONE >> 1
    while t:
        if t & 1:
            r = mulmod(r, base)
        base = mulmod(base, base)
        t >>= 1
    return r


def t_of_k(k, nt):
    """The exponent of image bit k (224 <= k < 8 nt) of an image of nt bytes."""
    L = nt - 32
    if k < 256:
        return 31 - (k - 224)
    m, b = (k - 256) // 8, (k - 256) % 8
    return 32 + 8 * (L - 1 - m) + (7 - b)


def k_of_t(t, nt):
    L = nt - 32
    if t < 32:
        return 224 + 31 - t
    u = t - 32
    return 256 + 8 * (L - 1 - u // 8) + (7 - u % 8)


def length_bit(k):
    byte, b = k // 8, k % 8
    return 32 <= byte <= 35 or byte == 41 or (byte, b) in ((38, 1), (39, 0))


def syndrome(img):
    """(S, nt) of an image given as exactly its nt bytes."""
    img = sm._u8(img)
    return oracle.crc32c(0, img[32:]) ^ int.from_bytes(bytes(img[28:32]), "little"), len(img)


def located_brute(img):
    """Every image bit k in [224, 8 nt) whose inversion makes stored == computed."""
    img = sm._u8(img).copy()
    crc, at, n = oracle.lib().oracle_crc32c, img.ctypes.data + 32, len(img) - 32  # (the bare call: one per bit)
    out = []
    for k in range(224, 8 * len(img)):
        img[k // 8] ^= 1 << (k % 8)
        if crc(0, at, n) == int.from_bytes(bytes(img[28:32]), "little"):
            out.append(k)
        img[k // 8] ^= 1 << (k % 8)
    return out


_BABY = {}


def _baby(m):
    if m not in _BABY:
        tab, g = {}, ONE
        for t in range(m):
            tab.setdefault(g, t)
            g = step(g)
        _BABY[m] = tab
    return _BABY[m]


def locate_t(S, npos, m=1 << 12):
    """The t < npos with g(t) == S, or None (npos < ORDER: at most one)."""
    if S == 0:
        return None
    baby, cur = _baby(m), S
    f = _BABY.setdefault(("giant", m), xpow(ORDER - m))  # x^-m
    for i in range(-(-npos // m)):
        if cur in baby:
            t = i * m + baby[cur]
            return t if t < npos else None
        cur = mulmod(cur, f)
    return None


def located_syndrome(img):
    S, nt = syndrome(img)
    t = locate_t(S, 32 + 8 * (nt - 32))
    return [] if t is None else [k_of_t(t, nt)]


def locate_bit(crc_computed, crc_stored, length):
    """crc32c_locate_bit: q = k - 224."""
    if length > SPAN_MAX:
        return NO_BIT
    t = locate_t(crc_computed ^ crc_stored, 32 + 8 * length)
    return NO_BIT if t is None else k_of_t(t, length + 32) - 224


def repair_one(buf, o, region=0, cfl=4, max_span=0, brute=False):
    """(ok, bit) of the image at o."""
    buf = sm._u8(buf)
    nt = sm.sane(buf, region or (1 << 62), o, cfl)
    if not nt or nt - 32 > (max_span or SPAN_DEFAULT):
        return 0, NO_BIT
    img = buf[o:o + nt]
    if syndrome(img)[0] == 0:
        return 1, NO_BIT
    ks = located_brute(img) if brute else located_syndrome(img)
    assert len(ks) <= 1
    if not ks or length_bit(ks[0]):
        return 0, NO_BIT
    k = ks[0]
    fixed = img.copy()
    fixed[k // 8] ^= 1 << (k % 8)
    nbytes = int.from_bytes(bytes(fixed[32:36]), "little")
    if nbytes < 2 or fixed[nt - 2] != 13 or fixed[nt - 1] != 10:
        return 0, NO_BIT
    return REPAIRED, k


def work(buf, offsets, region=0, cfl=4, max_span=0):
    """The work bound's sum: the spans of the images with S != 0 and L <= max_span."""
    buf, total = sm._u8(buf), 0
    for o in np.asarray(offsets).tolist():
        nt = sm.sane(buf, region or (1 << 62), int(o), cfl)
        if nt and nt - 32 <= (max_span or SPAN_DEFAULT) and syndrome(buf[int(o):int(o) + nt])[0]:
            total += nt - 32
    return total


def repair(buf, offsets, region=0, cfl=4, max_span=0, locate_only=False):
    """(ok, bit, nrepaired, nbad, the buffer afterwards) for distinct, disjoint images."""
    buf = sm._u8(buf)
    after = buf.copy()
    ok, bit = np.zeros(len(offsets), np.uint8), np.full(len(offsets), NO_BIT, np.uint64)
    assert work(buf, offsets, region, cfl, max_span) <= len(buf), "over the work bound: CRC32C_EWORK"
    for i, o in enumerate(np.asarray(offsets).tolist()):
        ok[i], b = repair_one(buf, int(o), region, cfl, max_span)
        bit[i] = b
        if ok[i] == REPAIRED and not locate_only:
            after[int(o) + b // 8] ^= 1 << (b % 8)
    return ok, bit, int((ok == REPAIRED).sum()), int((ok == 0).sum()), after


def boundary_bits(nt, most=8):
    """Image bits on both sides of every boundary of the search in an image of
    nt bytes: the first and last covered bit, stored-CRC bits 0 and 31, the
    first span bit, and the last position of each chunk with the first of the
    next (t = 8 CHUNK c - 1 and 8 CHUNK c), plus each byte step's edge there.
    An image of more than ``most`` chunks: its first and last ones' and three
    evenly spread ones' boundaries."""
    npos = 32 + 8 * (nt - 32)
    ts = {0, 31, 32, npos - 1, npos - 8, 7, 8}
    nchunks = -(-npos // (8 * CHUNK))
    cs = range(1, nchunks)
    if nchunks > most:
        cs = sorted({1, 2, nchunks // 4, nchunks // 2, 3 * nchunks // 4, nchunks - 2, nchunks - 1})
    for c in cs:
        for d in (-9, -8, -1, 0, 1, 7, 8):
            ts.add(8 * CHUNK * c + d)
    return sorted({k_of_t(t, nt) for t in ts if 0 <= t < npos})
