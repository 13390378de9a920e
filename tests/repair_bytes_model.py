"""The rule of crc32c_repair_bytes (include/crc32c_batch.h) restated over
numpy, with the CRCs from the CPU oracle.  Nothing here comes from the library.

The rule is stated twice.  ``located_brute`` is the rule as written: XOR each
byte of the stored CRC and the span with each of the 255 masks in turn,
recompute the CRC through the oracle, keep the pairs after which stored and
computed agree (for short images).  ``located_syndrome`` is its syndrome form:
S = computed ^ stored, V_0 = S, V_(j + 1) = V_j x^-8, and the step j < 4 + L at
which V_j is non-zero and confined to the register's top byte (for long ones).
``repair_one`` is the whole verdict of one image, ``repair`` of a list."""
import numpy as np

from tests import oracle
from tests import repair_model as rm
from tests import salvage_model as sm

NO_BIT = rm.NO_BIT
REPAIRED = rm.REPAIRED
SPAN_MAX = 190231     # 4 + L <= 190 235, the smallest distance at which two one-byte patterns share a syndrome
SPAN_DEFAULT = 0x10000
CHUNK = rm.CHUNK


def unstep(g):
    """g x^-1."""
    return (((g ^ rm.POLY) << 1) | 1) & 0xFFFFFFFF if g & rm.ONE else (g << 1) & 0xFFFFFFFF


def _unstep8(g):
    for _ in range(8):
        g = unstep(g)
    return g


INV8 = [_unstep8(b << 24) for b in range(256)]


def byte_of_step(j, length):
    """The codeword byte (p < 4: stored-CRC byte p, else span byte p - 4) of step j."""
    return 3 - j if j < 4 else length + 7 - j


step_of_byte = byte_of_step  # (the map is its own inverse)


def locate_step(S, steps):
    """(j, mask) of the first step j < steps whose V_j lies in the top byte, or None."""
    if S == 0:
        return None
    v = S
    for j in range(steps):
        if not v & 0x00FFFFFF:
            return j, v >> 24
        v = ((v << 8) & 0xFFFFFFFF) ^ INV8[v >> 24]
    return None


def locate_byte(crc_computed, crc_stored, length):
    """crc32c_locate_byte: (codeword byte, mask) or None."""
    if length > SPAN_MAX:
        return None
    hit = locate_step((crc_computed ^ crc_stored) & 0xFFFFFFFF, 4 + length)
    return None if hit is None else (byte_of_step(hit[0], length), hit[1])


def located_syndrome(img):
    """[(image byte, mask)] of an image given as exactly its nt bytes."""
    S, nt = rm.syndrome(img)
    hit = locate_step(S, 4 + nt - 32)
    return [] if hit is None else [(28 + byte_of_step(hit[0], nt - 32), hit[1])]


def located_brute(img):
    """Every (p, m), p an image byte in [28, nt), m in 1..255, such that the
    image with byte p XORed by m has stored == computed: all 255 (nt - 28)
    variants written out and their CRCs taken by the oracle."""
    img = sm._u8(img)
    nt = len(img)
    ps = np.repeat(np.arange(28, nt), 255)
    ms = np.tile(np.arange(1, 256, dtype=np.uint8), nt - 28)
    rows = np.tile(img, (len(ps), 1))
    rows[np.arange(len(ps)), ps] ^= ms
    crcs = oracle.batch(rows, np.arange(len(ps), dtype=np.uint64) * nt + 32, np.full(len(ps), nt - 32, np.uint64))
    stored = rows[:, 28:32].copy().view("<u4").reshape(-1)
    hit = np.flatnonzero(crcs == stored)
    return [(int(ps[i]), int(ms[i])) for i in hit]


def length_mask(p, m):
    """rm.length_bit for any bit that mask m inverts in image byte p."""
    return any(rm.length_bit(8 * p + b) for b in range(8) if m >> b & 1)


def repair_one(buf, o, region=0, cfl=4, max_span=0, brute=False):
    """(ok, byte, mask) of the image at o."""
    buf = sm._u8(buf)
    assert (max_span or SPAN_DEFAULT) <= SPAN_MAX, "CRC32C_EINVAL"
    nt = sm.sane(buf, region or (1 << 62), o, cfl)
    if not nt or nt - 32 > (max_span or SPAN_DEFAULT):
        return 0, NO_BIT, 0
    img = buf[o:o + nt]
    if rm.syndrome(img)[0] == 0:
        return 1, NO_BIT, 0
    pairs = located_brute(img) if brute else located_syndrome(img)
    assert len(pairs) <= 1
    if not pairs or length_mask(*pairs[0]):
        return 0, NO_BIT, 0
    p, m = pairs[0]
    fixed = img.copy()
    fixed[p] ^= m
    nbytes = int.from_bytes(bytes(fixed[32:36]), "little")
    if nbytes < 2 or fixed[nt - 2] != 13 or fixed[nt - 1] != 10:
        return 0, NO_BIT, 0
    return REPAIRED, p, m


def repair(buf, offsets, region=0, cfl=4, max_span=0, locate_only=False):
    """(ok, byte, mask, nrepaired, nbad, the buffer afterwards) for distinct, disjoint images."""
    buf = sm._u8(buf)
    after = buf.copy()
    n = len(offsets)
    ok, byte, mask = np.zeros(n, np.uint8), np.full(n, NO_BIT, np.uint64), np.zeros(n, np.uint8)
    assert rm.work(buf, offsets, region, cfl, max_span or SPAN_DEFAULT) <= len(buf), "over the work bound: CRC32C_EWORK"
    for i, o in enumerate(np.asarray(offsets).tolist()):
        ok[i], p, mask[i] = repair_one(buf, int(o), region, cfl, max_span)
        byte[i] = p
        if ok[i] == REPAIRED and not locate_only:
            after[int(o) + p] ^= mask[i]
    return ok, byte, mask, int((ok == REPAIRED).sum()), int((ok == 0).sum()), after
